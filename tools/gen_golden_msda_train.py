"""TEST INFRASTRUCTURE ONLY - records tests/golden/msda_train.npz from the UNMODIFIED reference module (models/ops/modules/ms_deform_attn.py,
found by oracle/ref_shims.py; it is absent where the tests run, so they read what this writes).

For the four cases tests/msda_train_ref.GOLDEN_CASES (f32 inputs, two of them with padding masks) the reference's MSDeformAttn runs in float64
with _export = True, so its own PyTorch core (grid_sample) runs on the CPU. Its Linears are set to selections: value_proj and output_proj are
identities, and the query carries, per head, that head's offsets and logits in the head's own d_model / M columns, which sampling_offsets and
attention_weights pick out with 0 / 1 weights - all exact, so the module's output and its gradients with respect to input_flatten, the query
and reference_points ARE out, grad_value, grad_offsets / grad_logits and grad_ref of the core. The reference has no level_start (it splits the
value rows by H W), so it gets the case's value rows without the gaps and the recorded grad_value has zeros there.

grad_ref of the engineered rows (a sample exactly on the border of the map) is recorded as the reference gives it; the tests leave those rows out:
grid_sample has a one-sided location derivative on the border itself, the operator's strict rule has none.

Recorded: every 1 + n // 300-th element of each of the five tensors in float64, and the reference's own float32 distance to float64 per tensor
in units of 2^-24 M_e (the measure of msda_train_ref.ratios). Run:  python tools/gen_golden_msda_train.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import msda_train_ref as R  # noqa: E402
from oracle import ref_shims  # noqa: E402

MAX_SAMPLES = 300


def sample_index(n):
    return np.arange(0, n, 1 + n // MAX_SAMPLES)


def run_reference(inp, ct):
    ref_shims.import_reference()
    from models.ops.modules.ms_deform_attn import MSDeformAttn
    case = inp["case"]
    B, Q, M, D, P = case["B"], case["Q"], case["M"], case["D"], case["P"]
    shapes, lsi, S = inp["shapes"], inp["lsi"], inp["S"]
    L, LP, d = shapes.shape[0], shapes.shape[0] * P, M * D
    assert 3 * LP <= D, "the query has D columns per head for 2 L P offsets and L P logits"
    mod = MSDeformAttn(d_model=d, n_levels=L, n_heads=M, n_points=P).to(ct)
    mod._export = True
    with torch.no_grad():
        for lin in (mod.value_proj, mod.output_proj):
            lin.weight.copy_(torch.eye(d, dtype=ct)); lin.bias.zero_()
        mod.sampling_offsets.weight.zero_(); mod.sampling_offsets.bias.zero_()
        mod.attention_weights.weight.zero_(); mod.attention_weights.bias.zero_()
        for m in range(M):
            for j in range(2 * LP):
                mod.sampling_offsets.weight[m * 2 * LP + j, m * D + j] = 1.0
            for i in range(LP):
                mod.attention_weights.weight[m * LP + i, m * D + 2 * LP + i] = 1.0
    keep = torch.cat([torch.arange(int(lsi[l]), int(lsi[l]) + int(shapes[l, 0] * shapes[l, 1])) for l in range(L)])
    query = torch.zeros(B, Q, M, D, dtype=ct)
    query[..., :2 * LP] = inp["off"].to(ct).reshape(B, Q, M, 2 * LP)
    query[..., 2 * LP:3 * LP] = inp["lg"].to(ct)
    query = query.reshape(B, Q, d).requires_grad_(True)
    flat = inp["value"].to(ct)[:, keep].reshape(B, len(keep), d).requires_grad_(True)
    ref = inp["ref"].to(ct, copy=True).requires_grad_(True)
    mask = None if inp["mask"] is None else inp["mask"][:, keep]
    start = torch.cat((shapes.new_zeros(1), (shapes[:, 0] * shapes[:, 1]).cumsum(0)[:-1]))
    out = mod(query, ref, flat, shapes, start, mask)
    out.backward(inp["go"].to(ct))
    gq = query.grad.reshape(B, Q, M, D)
    gv = torch.zeros(B, S, M, D, dtype=ct)
    gv[:, keep] = flat.grad.reshape(B, len(keep), M, D)
    got = dict(out=out, grad_value=gv, grad_offsets=gq[..., :2 * LP].reshape(B, Q, M, L, P, 2), grad_logits=gq[..., 2 * LP:3 * LP], grad_ref=ref.grad)
    return {t: v.detach().clone() for t, v in got.items()}


def main():
    if not ref_shims.reference_available():
        raise SystemExit("the reference is not present: this fixture is recorded from it")
    rec = {}
    for name in R.GOLDEN_CASES:
        case = next(c for c in R.CASES if c["name"] == name)
        inp = R.make_case(case, R.F32)
        g64, g32 = run_reference(inp, torch.float64), run_reference(inp, torch.float32)
        # a sample exactly at w_im = -1 or h_im = H: grid_sample has a one-sided derivative with respect to the location there, the operator's
        # rule (h_im > -1 && h_im < H, strict) gives none. Only grad_ref of the engineered rows sees it (their boxes have size 0)
        eng = inp["engineered"]
        g32["grad_ref"][eng] = R.ref64(inp)["grad_ref"][eng].float()
        dist = R.ratios(g32, R.ref64(inp))
        for t in R.TENSORS:
            flat = g64[t].reshape(-1).numpy()
            idx = sample_index(flat.size)
            rec[f"{name}/{t}/index"], rec[f"{name}/{t}/value"] = idx.astype(np.int64), flat[idx]
            rec[f"{name}/{t}/f32_distance"] = np.float64(dist[t])
        print(name, "reference f32 distance to f64, units of 2^-24 M_e:", {t: round(v, 2) for t, v in dist.items()})
    path = os.path.join(ROOT, "tests", "golden", "msda_train.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
