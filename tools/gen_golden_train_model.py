"""TEST INFRASTRUCTURE ONLY - records tests/golden/train_model.npz from the UNMODIFIED reference model (``models.build_model``, found by
oracle/ref_shims.py; it is absent where the tests run, so they read what this writes).

For each of the two reduced configurations of tests/train_model_ref.py (tiny: one level, d = 256, 2 points, images 128 x 128 and 96 x 128;
large: two levels, d = 384, 4 points, images 128 x 128 and 128 x 64; 4 ViT blocks, 10 queries, 3 groups, 2 decoder layers) the reference is
built, loaded with ``synth_state_dict(seed)``, put in train mode and run forward and backward on the CPU, once in float64 and once in float32,
on a NestedTensor of the two images (the second is padded). Its ``MSDeformAttn`` modules run their own PyTorch sampling core (``_export``: the
reference has no CPU build of its extension). The loss is sum(output * cotangent) over every tensor of the output dict.

Recorded from the float64 run: every output, the two-stage indices per group, the L2 norm and sum of every parameter's gradient, the whole
gradient of the tensors of ``train_model_ref.full_grad_keys``, the BatchNorm running statistics after the step; and for each of these the
figure of the float32 run against the float64 run (``train_model_ref.figures``). Neither weights nor images are stored.

The seed is the first for which the selection is DECIDED, by the rule of tools/gen_golden_two_stage.py: in every (group, image) the float64
gap between consecutive scores among the top nq + 1 is above 64 x the score bound of tests/two_stage_ref.py, evaluated on the ``memory`` the
float64 run handed its transformer. The float32 and float64 runs must return the same indices (asserted).
Run:  python tools/gen_golden_train_model.py            (searches the seeds: several minutes)
      python tools/gen_golden_train_model.py tiny=104 large=406      (the seeds the search found; the decided-selection rule is still asserted)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import train_model_ref as T  # noqa: E402
import two_stage_ref as R  # noqa: E402
from lwdetr_amd.synth import synth_state_dict  # noqa: E402
from oracle import ref_shims  # noqa: E402


def run_reference(name, seed, dtype):
    """-> (quantities, parameter names, what the transformer was handed) of the reference's train-mode step in ``dtype``."""
    models = ref_shims.import_reference()
    from models.ops.modules import MSDeformAttn
    from util.misc import nested_tensor_from_tensor_list
    args = T.args_of(name)
    model, _, _ = models.build_model(args)
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=seed), strict=True)
    for m in model.modules():
        if isinstance(m, MSDeformAttn):
            m._export = True
    model = model.to(dtype).train()
    seen, picked = {}, []
    model.transformer.register_forward_pre_hook(lambda _m, a: seen.update(srcs=a[0], masks=a[1]))
    real_topk = torch.topk

    def topk(*a, **k):
        out = real_topk(*a, **k)
        picked.append(out[1].clone())
        return out

    samples = nested_tensor_from_tensor_list([t.to(dtype) for t in T.images_of(name)])
    torch.topk = topk
    try:
        out = model(samples)
    finally:
        torch.topk = real_topk
    assert len(picked) == args.group_detr
    q, names = T.quantities(model, out, torch.stack(picked))
    return q, names, seen, model


def decided(name, seen, model):
    """The gap rule on the float64 run's memory."""
    args = T.args_of(name)
    G, nq = args.group_detr, args.num_queries
    memory = torch.cat([s.flatten(2).transpose(1, 2) for s in seen["srcs"]], 1).detach()
    mask = torch.cat([m.flatten(1) for m in seen["masks"]], 1)
    levels = [tuple(s.shape[-2:]) for s in seen["srcs"]]
    props, valid = R.proposals64(memory.shape[0], levels, mask, unsigmoid=False)
    tr = model.transformer
    st = lambda mods, a: torch.stack([getattr(mods[g], a).detach() for g in range(G)])
    inp = dict(dtype=torch.float32, memory=memory, rowvalid=valid, W_eo=st(tr.enc_output, "weight"), b_eo=st(tr.enc_output, "bias"),
               ln_w=st(tr.enc_output_norm, "weight"), ln_b=st(tr.enc_output_norm, "bias"), W_cls=st(tr.enc_out_class_embed, "weight"),
               b_cls=st(tr.enc_out_class_embed, "bias"))
    s64, M, Rr = R.scores_ref(inp)
    bound = R.score_bound(M, Rr)
    top, order = torch.sort(s64, dim=-1, descending=True, stable=True)
    gaps = top[..., :nq] - top[..., 1:nq + 1]
    b_here = torch.gather(bound, -1, order[..., :nq + 1])
    need = 64 * torch.maximum(b_here[..., :-1], b_here[..., 1:])
    return bool((gaps > need).all()), float((gaps / need).min()), order[..., :nq]


def first_decided_seed(name, limit=4096):
    """The first weight seed whose float64 forward gives a decided selection (forward only: one model, reloaded per seed)."""
    models = ref_shims.import_reference()
    from models.ops.modules import MSDeformAttn
    from util.misc import nested_tensor_from_tensor_list
    model, _, _ = models.build_model(T.args_of(name))
    for m in model.modules():
        if isinstance(m, MSDeformAttn):
            m._export = True
    model = model.double().train()
    seen = {}
    model.transformer.register_forward_pre_hook(lambda _m, a: seen.update(srcs=a[0], masks=a[1]))
    samples = nested_tensor_from_tensor_list([t.double() for t in T.images_of(name)])
    for seed in range(limit):
        sd = synth_state_dict(model.state_dict(), seed=seed)
        model.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, strict=True)
        with torch.no_grad():
            model(samples)
        if decided(name, seen, model)[0]:
            return seed
    raise SystemExit(f"{name}: no seed below {limit} gives a decided selection")


def main():
    if not ref_shims.reference_available():
        raise SystemExit("the reference is not present: this fixture is recorded from it")
    rec = {}
    for name in T.RECORDINGS:
        seed = first_decided_seed(name) if len(sys.argv) < 2 else int(dict(a.split("=") for a in sys.argv[1:])[name])
        q64, names, seen, model = run_reference(name, seed, torch.float64)
        ok, margin, own = decided(name, seen, model)
        assert ok, f"{name}: the selection of seed {seed} is not decided"
        assert torch.equal(q64["idx"], own), "the reference's top-k differs from the float64 restatement's"
        q32, names32, _, _ = run_reference(name, seed, torch.float32)
        assert names32 == names
        assert torch.equal(q32["idx"], q64["idx"]), "the float32 and float64 reference runs selected different tokens"
        fig = T.figures(q32, q64)
        print(f"{name}: seed {seed}, smallest gap / (64 x bound) {margin:.2f}; float32 figures per group:",
              {g: f"{v:.3e}" for g, v in T.group_figures(fig).items()})
        pre = name + "__"
        rec[pre + "seed"] = np.int64(seed)
        rec[pre + "param_names"] = np.array(names)
        for k, v in q64.items():
            rec[pre + "q__" + k] = v.numpy()
        for k, v in fig.items():
            rec[pre + "f__" + k] = np.float64(v)
    np.savez_compressed(T.GOLDEN_PATH, **rec)
    print("wrote", T.GOLDEN_PATH, os.path.getsize(T.GOLDEN_PATH), "bytes")


if __name__ == "__main__":
    main()
