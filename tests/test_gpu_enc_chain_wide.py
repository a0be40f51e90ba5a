"""GPU: the wide-class form of lwdetr_enc_chain (96 < ncls <= 384: enc_chain_kernel_wide, 12 class tiles; plan switch LWDETR_CHAIN_WIDE_CLS).

(1) the kernel against the fp32 torch restatement of the chain with the unfused launches' rounding points (tests/test_gpu_chain.py, same bounds: the
    per-element arithmetic is the same contraction over d), pad columns, the row maximum, canary rows behind every output;
(2) a level offset (rows of one level inside longer per-image sequences): everything outside the level's rows keeps its fill value;
(3) the narrow and the wide kernels bit for bit on what they share;
(4) the launch plan with and without the switch;
(5) 366-class models (dataset_file="o365") end to end against the fp32 CPU oracle, with the switch on and off."""
import json
import os

import pytest
import torch

import lwdetr_amd
from lwdetr_amd import kernels as K
from helpers import ROOT, chain_served_by

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL, CANARY = 7.0, 32


def _ln(x, g, b, eps):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), g, b, eps)


def _weights(g, d, k5, nl, ncls):
    r = lambda *s: torch.randn(*s, generator=g)
    w = dict(w_enc=r(d, d) / 16, b_enc=r(d) * 0.5, g_enc=1 + 0.1 * r(d), be_enc=0.1 * r(d), w_cls=r(ncls, d) / 16, b_cls=r(ncls),
             w_val=r(nl * d, d) / 16, b_val=r(nl * d) * 0.5)
    w["cv2"] = (r(d, k5) / 25, r(d) * 0.5, 1 + 0.1 * r(d), 0.1 * r(d)) if k5 else None
    return w


def _pack(w, d, dtype):
    return K.pack_enc_chain(d, dtype, w["w_enc"], w["b_enc"], w["g_enc"], w["be_enc"], w["w_cls"], w["b_cls"], w["w_val"], w["b_val"], cv2=w["cv2"])


def _reference(w, x, rowvalid, notpad, dtype, k5):
    """fp32 arithmetic on the 16-bit operands, every stage output rounded to the storage type (rowvalid / notpad per input row)."""
    T = lambda t: t.to(dtype).float()
    Wt = lambda t: t.to(dtype).float()
    xf = x.float()
    if k5:
        cv2 = w["cv2"]
        mem = T(_ln(T(torch.nn.functional.silu(xf @ Wt(cv2[0]).T + cv2[1])), cv2[2], cv2[3], 1e-6))
    else:
        mem = xf
    vals = T(mem @ Wt(w["w_val"]).T + w["b_val"]) * notpad[:, None].float()
    om = T(_ln(T((mem * rowvalid[:, None].float()) @ Wt(w["w_enc"]).T + w["b_enc"]), w["g_enc"], w["be_enc"], 1e-5))
    cls = T(om @ Wt(w["w_cls"]).T + w["b_cls"])
    return mem, vals, om, cls


def _launch(w, x, rowvalid_rows, notpad_rows, d, k5, dtype, nl, ncls, *, B, npix, S, lsi, ld_cls):
    """Runs lwdetr_enc_chain on x (B * npix, k5 or d); rowvalid_rows / notpad_rows (B * S,) in memory-row order. Every output has B * S rows
    + CANARY rows behind them, all pre-filled with FILL. Returns dict of the output tensors (with their canary rows)."""
    total = B * S
    full = lambda cols, dt=dtype: torch.full((total + CANARY, cols), FILL, dtype=dt, device=DEV)
    out = dict(memory=full(d), om=full(d), cls=full(ld_cls), cls_max=torch.full((total + CANARY,), FILL, dtype=torch.float32, device=DEV),
               values=[full(d) for _ in range(nl)])
    stream, vec = _pack(w, d, dtype)
    pad = lambda t: torch.cat([t, torch.ones(CANARY, dtype=torch.uint8)]).to(DEV)
    op = K.EncChainOp(x.to(DEV), k5 or d, k5, out["memory"] if k5 else None, out["om"], out["cls"], ld_cls, out["cls_max"], out["values"],
                      pad(rowvalid_rows), pad(notpad_rows), stream.to(DEV), vec.to(DEV), M=B * npix, d=d, npix=npix, S=S, lsi=lsi,
                      total_rows=total, ncls=ncls, eps_p=1e-6, eps_e=1e-5)
    form = f"enc_{'f16' if dtype == torch.float16 else 'bf16'}_d{d}_pf{int(bool(k5))}_{'narrow' if ncls <= 96 else 'wide'}"
    with chain_served_by(form):                                                                                     # (element-wise: test_gpu_chain_fp64.py)
        op()
    torch.cuda.synchronize()
    return out


def _close(got, ref, what, dtype, k=3.0):
    """The bounds of tests/test_gpu_chain.py:57-64."""
    ulp = 2.0 ** -10 if dtype == torch.float16 else 2.0 ** -7
    got = got.float().cpu()
    err = (got - ref).abs()
    bound = k * ulp * ref.abs().clamp(min=0.25)
    frac = (err > bound).float().mean().item()
    assert frac < 2e-3 and err.max().item() < 16 * k * ulp * max(1.0, ref.abs().max().item()), (what, frac, err.max().item())


# the ring wraps inside the class stage (48 / 72 pieces through 32 slots), a ragged last class tile (366, 97: one column of the fourth tile;
# 128: whole tiles, eight of them all pad) and 384 = all twelve tiles full, dead lanes in the last wave (every M here), several workgroups
CASES = [(256, 640, torch.float16, 2, 100, 366), (256, 0, torch.bfloat16, 1, 333, 97), (384, 0, torch.float16, 1, 77, 384),
         (384, 0, torch.bfloat16, 2, 160, 366), (256, 640, torch.bfloat16, 3, 50, 128)]


@pytest.mark.parametrize("d,k5,dtype,B,npix,ncls", CASES)
def test_wide_enc_chain_matches_torch(d, k5, dtype, B, npix, ncls):
    g = torch.Generator().manual_seed(d + k5 + npix + ncls)
    nl, M = 3, B * npix
    w = _weights(g, d, k5, nl, ncls)
    x = (torch.randn(M, k5 or d, generator=g) * (1.0 if k5 else 1.5)).to(dtype)
    rowvalid = (torch.rand(M, generator=g) > 0.3).to(torch.uint8)
    notpad = (torch.rand(M, generator=g) > 0.2).to(torch.uint8)
    mem, vals, om, cls = _reference(w, x, rowvalid, notpad, dtype, k5)
    out = _launch(w, x, rowvalid, notpad, d, k5, dtype, nl, ncls, B=B, npix=npix, S=npix, lsi=0, ld_cls=384)
    if k5:
        _close(out["memory"][:M], mem, "memory", dtype)
    else:
        assert (out["memory"] == FILL).all()                   # not an output of this form
    for i in range(nl):
        _close(out["values"][i][:M], vals[:, i * d:(i + 1) * d], f"values[{i}]", dtype)
        assert (out["values"][i][:M].float().cpu()[notpad == 0] == 0).all()
    _close(out["om"][:M], om, "om", dtype, k=4.0)
    clso = out["cls"][:M]
    _close(clso[:, :ncls], cls, "cls", dtype, k=6.0)
    assert (clso[:, ncls:] == 0).all()                         # pad columns [ncls, 384): zero weights and biases
    # the row maximum is the maximum of the kernel's own (rounded) class logits over the real classes, exactly
    assert torch.equal(out["cls_max"][:M], clso[:, :ncls].float().max(1).values)
    for name in ("memory", "om", "cls", "cls_max"):
        assert (out[name][M:] == FILL).all(), f"canary rows behind {name}"
    for i in range(nl):
        assert (out["values"][i][M:] == FILL).all(), f"canary rows behind values[{i}]"


def test_wide_enc_chain_writes_only_the_rows_of_its_level():
    """Rows of one level inside longer per-image sequences: input row m -> memory row b * S + lsi + m % npix. The row flags are read there too."""
    d, k5, dtype, B, npix, ncls, nl = 384, 0, torch.float16, 2, 150, 366, 3
    S, lsi = npix + 40, 40
    g = torch.Generator().manual_seed(99)
    M = B * npix
    w = _weights(g, d, k5, nl, ncls)
    x = (torch.randn(M, d, generator=g) * 1.5).to(dtype)
    rowvalid = (torch.rand(M, generator=g) > 0.3).to(torch.uint8)
    notpad = (torch.rand(M, generator=g) > 0.2).to(torch.uint8)
    dest = (torch.arange(M) // npix) * S + lsi + torch.arange(M) % npix
    # flags in memory-row order, zero outside the level: read at the input row's index instead, they would zero rows that the reference keeps
    rv_rows, np_rows = torch.zeros(B * S, dtype=torch.uint8), torch.zeros(B * S, dtype=torch.uint8)
    rv_rows[dest], np_rows[dest] = rowvalid, notpad
    _, vals, om, cls = _reference(w, x, rowvalid, notpad, dtype, k5)
    out = _launch(w, x, rv_rows, np_rows, d, k5, dtype, nl, ncls, B=B, npix=npix, S=S, lsi=lsi, ld_cls=384)
    inside = torch.zeros(B * S + CANARY, dtype=torch.bool)
    inside[dest] = True
    for i in range(nl):
        _close(out["values"][i][dest.to(DEV)], vals[:, i * d:(i + 1) * d], f"values[{i}]", dtype)
    _close(out["om"][dest.to(DEV)], om, "om", dtype, k=4.0)
    clso = out["cls"][dest.to(DEV)]
    _close(clso[:, :ncls], cls, "cls", dtype, k=6.0)
    assert (clso[:, ncls:] == 0).all()
    assert torch.equal(out["cls_max"][dest.to(DEV)], clso[:, :ncls].float().max(1).values)
    outside = (~inside).to(DEV)
    assert int(outside.sum()) == B * 40 + CANARY
    for name in ("om", "cls", "cls_max", "memory"):
        assert (out[name][outside] == FILL).all(), name
    for i in range(nl):
        assert (out["values"][i][outside] == FILL).all(), i
    assert (out["memory"] == FILL).all()


@pytest.mark.parametrize("d,k5,dtype", [(256, 640, torch.float16), (256, 0, torch.bfloat16), (384, 0, torch.float16)])
def test_narrow_and_wide_kernels_agree_bit_for_bit(d, k5, dtype):
    """The same inputs through enc_chain_kernel (91 classes) and enc_chain_kernel_wide (those 91 rows of w_cls + 275 more): memory, values,
    output_memory and class columns 0 .. 90 are the same bits - every stage before the class stage is the same code, and a class tile is the
    same instruction sequence on the same operands."""
    g = torch.Generator().manual_seed(d + k5)
    nl, B, npix = 3, 2, 210
    M = B * npix
    wn = _weights(g, d, k5, nl, 91)
    ww = dict(wn)
    ww["w_cls"] = torch.cat([wn["w_cls"], torch.randn(275, d, generator=g) / 16])
    ww["b_cls"] = torch.cat([wn["b_cls"], torch.randn(275, generator=g)])
    x = (torch.randn(M, k5 or d, generator=g) * (1.0 if k5 else 1.5)).to(dtype)
    rowvalid = (torch.rand(M, generator=g) > 0.3).to(torch.uint8)
    notpad = (torch.rand(M, generator=g) > 0.2).to(torch.uint8)
    kw = dict(B=B, npix=npix, S=npix, lsi=0)
    a = _launch(wn, x, rowvalid, notpad, d, k5, dtype, nl, 91, ld_cls=96, **kw)
    b = _launch(ww, x, rowvalid, notpad, d, k5, dtype, nl, 366, ld_cls=384, **kw)
    assert torch.equal(a["memory"], b["memory"])
    assert (a["memory"][:M] != FILL).any() == bool(k5)
    for i in range(nl):
        assert torch.equal(a["values"][i], b["values"][i]), i
    assert torch.equal(a["om"], b["om"]) and (a["om"][:M] != FILL).any()
    assert torch.equal(a["cls"][:M, :91], b["cls"][:M, :91])
    assert (a["cls"][:M, 91:] == 0).all() and (b["cls"][:M, 91:366] != 0).any() and (b["cls"][:M, 366:] == 0).all()
    assert torch.equal(a["cls_max"][:M], a["cls"][:M, :91].float().max(1).values)
    assert torch.equal(b["cls_max"][:M], b["cls"][:M, :366].float().max(1).values)
    assert (b["cls_max"][:M] >= a["cls_max"][:M]).all()


# ------------------------------------------------------------------------------------------------------------------------- plan and model
def _o365_model(size, dtype, dataset_file="o365", seed=0):
    from lwdetr_amd.synth import synth_state_dict
    cfg = lwdetr_amd.get_args(size, dataset_file=dataset_file)
    model, _, post = lwdetr_amd.build_model(cfg)
    sd = synth_state_dict(model.state_dict(), seed=seed)
    model.load_state_dict(sd)
    return cfg, sd, model.to(DEV).to(dtype).eval(), post


def _op_names(plan):
    return [type(op).__name__ for ops in (plan.ops_backbone, plan.ops_enc, plan.ops_sel, plan.ops_dec) for op in ops]


def test_plan_takes_the_wide_chain_only_behind_its_switch(monkeypatch):
    monkeypatch.setenv("LWDETR_CHAIN", "1")
    plans = {}
    for ds in ("o365", "coco"):
        _, _, model, _ = _o365_model("tiny", torch.float16, ds)
        for sw in ("1", None):
            if sw is None:
                monkeypatch.delenv("LWDETR_CHAIN_WIDE_CLS")
            else:
                monkeypatch.setenv("LWDETR_CHAIN_WIDE_CLS", sw)
            plans[ds, sw] = model._plan(2, 192, 256, private=True)
    on, off = plans["o365", "1"], plans["o365", None]
    assert on.ncls == off.ncls == 366
    assert on.use_chain and sum(isinstance(op, K.EncChainOp) for op in on.ops_enc) == 1 and on.ldc_enc == 384
    assert tuple(on.enc_cls.shape) == (on.B * on.S, 384)
    assert not off.use_chain and not any(isinstance(op, K.EncChainOp) for op in off.ops_enc) and off.ldc_enc == off.ldc == 368
    assert "GemmOp" in [type(op).__name__ for op in off.ops_enc] and "LayerNormOp" in [type(op).__name__ for op in off.ops_enc]
    a, b = plans["coco", "1"], plans["coco", None]
    assert a.ncls == 91 and a.use_chain and b.use_chain and a.ldc_enc == b.ldc_enc == 96
    assert _op_names(a) == _op_names(b)
    assert sum(isinstance(op, K.EncChainOp) for op in a.ops_enc) == 1


# fp16 bounds of the matching 91-class padded cases of tests/test_gpu_model.py:231 (logits, boxes). The plan without the switch is inside them
# too, so they stand as they are. Measured on MI355X against the fp32 CPU oracle (parity_o365_*.json, see LWDETR_PARITY_DIR below), max |error| of
# pred_logits / enc_logits / pred_boxes / enc_boxes:
#   small/o365 padded (448, 512), (320, 384):  switch off 0.0211 / 0.0082 / 0.00188 / 0.00037, switch on 0.0211 / 0.0082 / 0.00139 / 0.00037
#   large/o365 padded (384, 320), (256, 320):  switch off 0.0160 / 0.0085 / 0.00148 / 0.00066, switch on 0.0160 / 0.0085 / 0.00173 / 0.00066
O365_CASES = {"small": ([(448, 512), (320, 384)], 0.05, 0.005), "large": ([(384, 320), (256, 320)], 0.09, 0.008)}


@pytest.mark.parametrize("size", list(O365_CASES))
def test_o365_model_through_the_wide_chain(size, monkeypatch):
    """366-class models, fp16, padded batches, LWDETR_CHAIN=1, teacher-forced selection from the fp32 CPU oracle on the same state dict: the plan with
    the wide chain and the plan without it (separate launches: the behaviour without the switch) agree on every stage the chain replaces, and the
    outputs with the switch on are within the 16-bit bounds of the 91-class cases."""
    from oracle import lwdetr_torch as O
    from lwdetr_amd.models.nested import NestedTensor
    from lwdetr_amd.synth import synth_images
    dims, tol_logit, tol_box = O365_CASES[size]
    hmax, wmax = max(d[0] for d in dims), max(d[1] for d in dims)
    images = synth_images(len(dims), hmax, wmax, seed=1234)
    mask = torch.ones(len(dims), hmax, wmax, dtype=torch.bool)
    for i, (h, w) in enumerate(dims):
        images[i, :, h:, :] = 0
        images[i, :, :, w:] = 0
        mask[i, :h, :w] = False
    monkeypatch.setenv("LWDETR_CHAIN", "1")
    dtype = torch.float16
    cfg, sd, model, post = _o365_model(size, dtype)
    with torch.no_grad():
        exp = O.forward(sd, cfg, images, mask)
    assert exp["pred_logits"].shape[-1] == 366
    forced = exp["topk_idx"].to(DEV)
    outs = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("LWDETR_CHAIN_WIDE_CLS", sw)
        model.invalidate_cache()                                  # the switch is read when a plan is built
        col = {}
        outs[sw] = (model(NestedTensor(images.to(DEV).to(dtype), mask.to(DEV)), _collect=col, _forced_topk=forced), col)
        plan = next(iter(model._plans.values()))
        assert plan.use_chain == (sw == "1") and plan.ncls == 366
        assert sum(isinstance(op, K.EncChainOp) for op in plan.ops_enc) == (1 if sw == "1" else 0)
    err = {}
    for sw, (out, _) in outs.items():
        e = lambda a, b: (a.float().cpu() - b).abs().max().item()
        err[sw] = dict(pred_logits=e(out["pred_logits"], exp["pred_logits"]), pred_boxes=e(out["pred_boxes"], exp["pred_boxes"]),
                       enc_logits=e(out["enc_outputs"]["pred_logits"], exp["enc_outputs"]["pred_logits"]),
                       enc_boxes=e(out["enc_outputs"]["pred_boxes"], exp["enc_outputs"]["pred_boxes"]))
    print(f"o365 {size}: switch off {err['0']} | switch on {err['1']}")
    outdir = os.environ.get("LWDETR_PARITY_DIR")               # where a run keeps its measured figures (relative to the repository root), if anywhere
    if outdir:
        outdir = os.path.join(ROOT, outdir)
        os.makedirs(outdir, exist_ok=True)
        with open(os.path.join(outdir, f"parity_o365_{size}_padded_float16.json"), "w") as f:
            json.dump({"wide_chain_off": err["0"], "wide_chain_on": err["1"], "bounds": {"logits": tol_logit, "boxes": tol_box}}, f)
    (out, col), (_, col0) = outs["1"], outs["0"]
    # the two launch plans agree to 16-bit noise on every stage the chain replaces (tests/test_gpu_model.py:256-259)
    for k in ("memory", "om"):
        a, b = col[k].float(), col0[k].float()
        assert (a - b).abs().max().item() <= 0.03 * max(1.0, b.abs().max().item()), k
    assert (col["enc.class_max"] - col0["enc.class_max"]).abs().max().item() < 0.06
    # PostProcess on the wide plan's outputs: labels up to 365, the scores of the oracle's own post-processing
    sizes = torch.tensor([[480.0, 640.0]] * len(dims))
    res = post["bbox"](out, sizes.to(DEV))
    labels = torch.stack([r["labels"] for r in res])
    assert tuple(labels.shape) == (len(dims), cfg.num_select) and int(labels.min()) >= 0 and int(labels.max()) <= 365
    e1 = err["1"]
    assert max(e1["pred_logits"], e1["enc_logits"]) < tol_logit, err
    assert max(e1["pred_boxes"], e1["enc_boxes"]) < tol_box, err
    # sorted scores, rank by rank: two sorted lists differ by at most the largest element-wise difference, and |d sigmoid| <= |d logit| / 4
    exp_scores = torch.stack([r["scores"] for r in O.postprocess(exp, sizes, cfg.num_select)])
    assert (torch.stack([r["scores"] for r in res]).float().cpu() - exp_scores).abs().max().item() < tol_logit / 4
