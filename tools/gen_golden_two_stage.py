"""TEST INFRASTRUCTURE ONLY - records tests/golden/two_stage_train.npz from the UNMODIFIED reference ``Transformer`` (models/transformer.py,
found by oracle/ref_shims.py; it is absent where the tests run, so they read what this writes).

The reference Transformer is built with two_stage=True, group_detr = 2, num_queries = 8, d_model = 256, one 9 x 11 level, bbox_reparam=True,
gets the two heads ``LWDETR.__init__`` attaches (enc_out_class_embed: Linear(256, 91), enc_out_bbox_embed: MLP(256, 256, 4, 3)) and runs in
train mode in float32 on the CPU on a batch of two images, image 1 padded; its ``decoder`` is replaced by a recorder. Every weight and input
is an int8 multiple of 2^-7 (stored as int8), so the file is small and the values are exact in every dtype.

Recorded: the inputs, the indices its torch.topk returned per group, memory_ts, boxes_ts, and what the decoder was handed (tgt, the reparametrised
reference points, memory, mask, pos, level_start_index, spatial_shapes, valid_ratios).

The seed is the first for which the selection is DECIDED, so that any correct implementation must reproduce the indices (asserted here):
  - in every (g, b), the float64 gap between consecutive scores among the top nq + 1 is above 64 x the score bound of tests/two_stage_ref.py;
  - no valid row ties with the invalid rows' constant score inside the top nq + 1 (the same gap rule covers it: an invalid row may appear
    there only once).
Run:  python tools/gen_golden_two_stage.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import two_stage_ref as R  # noqa: E402
from oracle import ref_shims  # noqa: E402

CASE = R.GOLDEN_CASE
SCALE = 2.0 ** -7


class Recorder(nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = None

    def forward(self, tgt, memory, **kw):
        self.seen = dict(tgt=tgt, memory=memory, **kw)
        return tgt.unsqueeze(0), kw["refpoints_unsigmoid"].unsqueeze(0)


def quantised(gen, shape, spread):
    """int8 values in [-spread, spread]: the tensor is value * 2^-7."""
    return torch.randint(-spread, spread + 1, shape, generator=gen, dtype=torch.int8)


def make_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    d, G, B, nq, ncls = CASE["d"], CASE["G"], CASE["B"], CASE["nq"], CASE["ncls"]
    (h, w), = CASE["levels"]
    q = dict(src=quantised(gen, (B, d, h, w), 127), pos=quantised(gen, (B, d, h, w), 64), refpoint=quantised(gen, (G * nq, 4), 32),
             query_feat=quantised(gen, (G * nq, d), 64),
             W_eo=quantised(gen, (G, d, d), 13), b_eo=quantised(gen, (G, d), 13), ln_w=quantised(gen, (G, d), 13),
             ln_b=quantised(gen, (G, d), 13), W_cls=quantised(gen, (G, ncls, d), 13), b_cls=quantised(gen, (G, ncls), 64),
             W_box0=quantised(gen, (G, d, d), 13), b_box0=quantised(gen, (G, d), 13), W_box1=quantised(gen, (G, d, d), 13),
             b_box1=quantised(gen, (G, d), 13), W_box2=quantised(gen, (G, 4, d), 6), b_box2=quantised(gen, (G, 4), 13))
    return q


as_float, ref_inputs = R.golden_floats, R.golden_inputs


def decided(inp):
    s64, M, Rr = R.scores_ref(inp)
    bound = R.score_bound(M, Rr)
    nq = CASE["nq"]
    top, order = torch.sort(s64, dim=-1, descending=True, stable=True)
    gaps = top[..., :nq] - top[..., 1:nq + 1]
    b_here = torch.gather(bound, -1, order[..., :nq + 1])
    need = 64 * torch.maximum(b_here[..., :-1], b_here[..., 1:])
    return bool((gaps > need).all()), float((gaps / need).min())


def run_reference(f):
    ref_shims.import_reference()
    from models.transformer import MLP, Transformer
    d, G, nq, ncls = CASE["d"], CASE["G"], CASE["nq"], CASE["ncls"]
    tr = Transformer(d_model=d, sa_nhead=8, ca_nhead=8, num_queries=nq, num_decoder_layers=1, dim_feedforward=64, group_detr=G, two_stage=True,
                     num_feature_levels=1, dec_n_points=2, lite_refpoint_refine=True, bbox_reparam=True)
    tr.enc_out_bbox_embed = nn.ModuleList([MLP(d, d, 4, 3) for _ in range(G)])
    tr.enc_out_class_embed = nn.ModuleList([nn.Linear(d, ncls) for _ in range(G)])
    with torch.no_grad():
        for g in range(G):
            tr.enc_output[g].weight.copy_(f["W_eo"][g]); tr.enc_output[g].bias.copy_(f["b_eo"][g])
            tr.enc_output_norm[g].weight.copy_(f["ln_w"][g]); tr.enc_output_norm[g].bias.copy_(f["ln_b"][g])
            tr.enc_out_class_embed[g].weight.copy_(f["W_cls"][g]); tr.enc_out_class_embed[g].bias.copy_(f["b_cls"][g])
            for i in range(3):
                tr.enc_out_bbox_embed[g].layers[i].weight.copy_(f[f"W_box{i}"][g]); tr.enc_out_bbox_embed[g].layers[i].bias.copy_(f[f"b_box{i}"][g])
    rec = Recorder()
    tr.decoder = rec
    tr.train()
    (h, w), = CASE["levels"]
    mask = R.mask_of(CASE).view(CASE["B"], h, w)
    picked = []
    real_topk = torch.topk

    def topk(*a, **k):
        out = real_topk(*a, **k)
        picked.append(out[1].clone())
        return out

    torch.topk = topk
    try:
        with torch.no_grad():
            hs, refs, memory_ts, boxes_ts = tr([f["src"]], [mask], [f["pos"]], f["refpoint"], f["query_feat"])
    finally:
        torch.topk = real_topk
    assert len(picked) == G
    return dict(idx=torch.stack(picked), memory_ts=memory_ts, boxes_ts=boxes_ts, seen=rec.seen)


def main():
    if not ref_shims.reference_available():
        raise SystemExit("the reference is not present: this fixture is recorded from it")
    for seed in range(200):
        q = make_inputs(seed)
        f = as_float(q)
        ok, margin = decided(ref_inputs(f))
        if ok:
            break
    else:
        raise SystemExit("no seed gives a decided selection")
    print("seed", seed, "smallest gap / (64 x bound):", round(margin, 2))
    out = run_reference(f)
    inp = ref_inputs(f)
    s64, _, _ = R.scores_ref(inp)
    assert torch.equal(out["idx"], R.stable_topk(s64, CASE["nq"])), "the reference's own top-k differs from the float64 restatement's"
    seen = out["seen"]
    rec = {f"in_{k}": v.numpy() for k, v in q.items()}
    rec.update(seed=np.int64(seed), idx=out["idx"].numpy(), memory_ts=out["memory_ts"].numpy(), boxes_ts=out["boxes_ts"].numpy(),
               dec_tgt=seen["tgt"].numpy(), dec_refpoints=seen["refpoints_unsigmoid"].numpy(),
               dec_memory_is_input=np.bool_(torch.equal(seen["memory"], inp["memory"])),
               dec_mask=seen["memory_key_padding_mask"].numpy(), dec_pos_is_input=np.bool_(torch.equal(seen["pos"], f["pos"].flatten(2).transpose(1, 2))),
               dec_level_start_index=seen["level_start_index"].numpy(), dec_spatial_shapes=seen["spatial_shapes"].numpy(),
               dec_valid_ratios=seen["valid_ratios"].numpy())
    path = os.path.join(ROOT, "tests", "golden", "two_stage_train.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
