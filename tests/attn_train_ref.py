"""Shared by test_attn_train_host.py (CPU) and test_gpu_attn_train.py (GPU): the cases, the float64 evaluation, the reference formulation
in dtype T, the per-element magnitudes and the bound of the differentiable fused attention (csrc/attention_train.hip).

Operation, per (batch, head), scale c:  s = c q k^T, a = softmax_k(s), o = a v, lse = log sum_k exp(s);
  D = rowsum(do o), p = exp(s - lse), dv = p^T do, dp = do v^T, ds = p (dp - D), dq = c ds k, dk = c ds^T q.

Bound, for every element e of o, dq, dk, dv:   |got - ref64| <= 4 C[T][tensor] u_T M_e + half_ulp_T(|ref64_e|),
u_T = 2^-24 / 2^-11 / 2^-8, with the magnitudes M_o = a |v|, M_dv = a^T |do|, A = a (|do| |v|^T + rowsum(a |do| |v|^T)), M_dq = c A |k|,
M_dk = c A^T |q|, all in float64. C[T][tensor] (C_MEASURED) is the largest |ref_T - ref64| / (u_T M_e) that the reference formulation - the
materialised-score computation in dtype T under torch autograd on the CPU - reaches over the cases below; test_attn_train_host.py measures
it again and pins the table. The factor 4 is the project's margin over a measured reference.
lse: |got - ref64| <= 4 u_f32 (|lse| + max_k |s|) + TRANS_F32 + half_ulp_f32(|lse|), TRANS_F32 = 4 x 7.327 x 2^-23 the measured exp / log
deviation of tests/test_gpu_attention_fp64.py (a relative deviation of the sum of exponentials is an absolute one of its logarithm).

Cases: N(0, 1) operands rounded to T. Extra weight sits on the keys at tile edges (first / last of a 16-key tile and of a 32- / 64-key loop
step, the last real key, the first key of the ragged tile and of the ragged step, both sides of the one-launch threshold): such a key is made parallel to a query that is itself at a tile edge,
with a score of log N + 2, so that a dropped or doubled key or query moves its row by far more than the bound. One query row per case is scaled
until its scores spread over at least 200 nats (> 2^8 in the log2 domain) and its largest score stands 40 nats above the next (scores capped at
2000): the running maximum has to be rescaled by more than 2^8 whenever a later tile brings a new one, a missed rescale leaves a stale weight of
1 in the row, and the row's weights are the same one-hot vector in every number format, so that the reference formulation's 16-bit scores
(absolute error near 0.5 at a score of 200) do not turn C[T] into the error of that one row.
"""
import math

import torch

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = (F32, F16, BF16)
NAME = {F32: "f32", F16: "f16", BF16: "bf16"}
U = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}
PREC = {F32: 24, F16: 11, BF16: 8}
EMIN = {F32: -126, F16: -14, BF16: -126}
TRANS_F32 = 4 * 7.327 * 2.0 ** -23
TENSORS = ("o", "dq", "dk", "dv")
TILE = 16                       # the MFMA tile of every form of attention_train.hip; a loop step is 4 tiles at hd 16 / 32, 2 at hd 64
ONE_LAUNCH_MAX_N = 256          # backward: one launch up to here, dot + dkdv + dq above
SENT = 1234.0
GUARD = 3

# Largest |ref_T - ref64| / (u_T M_e) of the reference formulation over CASES (measure_constants(); pinned by test_attn_train_host.py).
C_MEASURED = {
    F32: {"o": 37.41, "dq": 3.642, "dk": 1.770, "dv": 16.56},
    F16: {"o": 2.018, "dq": 0.4162, "dk": 0.3005, "dv": 1.589},
    BF16: {"o": 2.496, "dq": 0.4439, "dk": 0.4858, "dv": 3.649},
}


def _case(N, hd, B=1, heads=2, distinct=False, only=None):
    return dict(N=N, hd=hd, B=B, heads=heads, distinct=distinct, only=only, name=f"N{N}_hd{hd}_B{B}_h{heads}" + ("_distinct" if distinct else ""))


# the issue's list; T - 1, T, T + 1, 2 T + 3 for the 16-row MFMA tile and for the loop step of every form (64 rows at hd 16 / 32, 32 at hd 64);
# both sides of the one-launch threshold; the recipes' 784 and (once, f32) 3136. Head sizes rotate so that every (form, dtype, hd)
# instantiation is served by some case
CASES = [_case(1, 16), _case(2, 32), _case(15, 64), _case(16, 16), _case(17, 32), _case(31, 64), _case(32, 64), _case(33, 64), _case(33, 16),
         _case(35, 32), _case(49, 64), _case(63, 32), _case(64, 16), _case(65, 32), _case(67, 64), _case(100, 16), _case(131, 16), _case(196, 64),
         _case(256, 32), _case(257, 16), _case(300, 64), _case(784, 32), _case(40, 32, B=2, heads=3, distinct=True),
         _case(3136, 16, heads=1, only=F32)]


def cases_for(dtype):
    return [c for c in CASES if c["only"] in (None, dtype)]


def half_ulp(v, dtype):
    """Half the spacing of `dtype` at |v| (float64 tensor)."""
    _, e = torch.frexp(v.abs().double())
    e = (e - 1).clamp_min(EMIN[dtype])
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), e - PREC[dtype])


def edge_indices(N):
    want = [0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 4 * TILE - 1, 4 * TILE, N - 1, (N - 1) // TILE * TILE, (N - 1) // TILE * TILE - 1,
            (N - 1) // (2 * TILE) * 2 * TILE, (N - 1) // (4 * TILE) * 4 * TILE, ONE_LAUNCH_MAX_N - 1, ONE_LAUNCH_MAX_N]
    out = []
    for i in want:
        if 0 <= i < N and i not in out:
            out.append(i)
    return out


_CACHE = {}


def cached(key, fn):
    """Cases and references are computed once and shared between the tests that need them; nothing modifies them."""
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def make_case(case, dtype):
    """-> dict with q, k, v (B, heads, N, hd) and do (B, N, heads*hd), CPU tensors of `dtype`, and scale."""
    def build():
        B, heads, N, hd = case["B"], case["heads"], case["N"], case["hd"]
        g = torch.Generator().manual_seed(1000 * N + hd + (7 if case["distinct"] else 0))
        q, k, v = (torch.randn(B, heads, N, hd, generator=g, dtype=torch.float64) for _ in range(3))
        do = torch.randn(B, N, heads * hd, generator=g, dtype=torch.float64)
        scale = hd ** -0.5
        q, k = q.to(dtype).double(), k.to(dtype).double()
        edges = edge_indices(N)
        for i, key in enumerate(edges):                                    # a heavy key per edge, seen by a query that is at an edge too
            qi = edges[(i + 1) % len(edges)]
            b, h = i % B, (i // B) % heads
            c = (math.log(N) + 2.0) / (scale * float((q[b, h, qi] ** 2).sum()))
            k[b, h, key] = (q[b, h, qi] * c).to(dtype).double()
        if N >= 2:                                                          # the rescale row: scores spread over 200 nats
            cand = [i for i in range(N) if i not in edges] or list(range(N))
            for b in range(B):
                for h in range(heads):
                    s = scale * (q[b, h, cand] @ k[b, h].T)
                    top = torch.topk(s, 2, dim=-1).values
                    f = torch.maximum(200.0 / (s.amax(-1) - s.amin(-1)).clamp_min(1e-3), 40.0 / (top[:, 0] - top[:, 1]).clamp_min(1e-3))
                    i = int((f * s.abs().amax(-1)).argmin())            # the row that needs the smallest scores for it
                    q[b, h, cand[i]] = q[b, h, cand[i]] * min(float(f[i]), 2000.0 / float(s[i].abs().max()))
        return dict(q=q.to(dtype), k=k.to(dtype), v=v.to(dtype), do=do.to(dtype), scale=scale, case=case, dtype=dtype)
    return cached(("case", case["name"], dtype), build)


def _do_heads(do, heads):
    B, N, C = do.shape
    return do.reshape(B, N, heads, C // heads).permute(0, 2, 1, 3)


def _merge(t):
    """(B, heads, N, hd) -> (B, N, heads*hd)"""
    B, H, N, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * D)


def ref64(inp):
    """The float64 evaluation on the operands as stored, with the magnitudes: dict o (B, N, C), lse (B, heads, N), dq / dk / dv (B, heads, N, hd),
    M_o, M_dq, M_dk, M_dv in the same shapes, smax (B, heads, N)."""
    def build():
        q, k, v = inp["q"].double(), inp["k"].double(), inp["v"].double()
        heads, c = q.shape[1], inp["scale"]
        do = _do_heads(inp["do"].double(), heads)
        s = c * (q @ k.transpose(-1, -2))
        lse = torch.logsumexp(s, -1)
        a = torch.exp(s - lse[..., None])
        o = a @ v
        D = (do * o).sum(-1, keepdim=True)
        dp = do @ v.transpose(-1, -2)
        ds = a * (dp - D)
        adp = do.abs() @ v.abs().transpose(-1, -2)
        A = a * (adp + (a * adp).sum(-1, keepdim=True))
        return dict(o=_merge(o), lse=lse, dq=c * (ds @ k), dk=c * (ds.transpose(-1, -2) @ q), dv=a.transpose(-1, -2) @ do,
                    M_o=_merge(a @ v.abs()), M_dq=c * (A @ k.abs()), M_dk=c * (A.transpose(-1, -2) @ q.abs()), M_dv=a.transpose(-1, -2) @ do.abs(),
                    smax=s.abs().amax(-1))
    return cached(("ref64", inp["case"]["name"], inp["dtype"]), build)


def formulation(q, k, v, scale):
    """The reference formulation: scores materialised, in the operands' dtype. (B, heads, N, hd) x 3 -> (B, N, heads*hd)."""
    w = ((q * scale) @ k.transpose(-2, -1)).softmax(dim=-1)
    return _merge(w @ v)


def ref_T(inp):
    """The reference formulation in dtype T under torch autograd (CPU): o, dq, dk, dv."""
    def build():
        q, k, v = (inp[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
        o = formulation(q, k, v, inp["scale"])
        o.backward(inp["do"])
        return dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad)
    return cached(("refT", inp["case"]["name"], inp["dtype"]), build)


def ratios(got, r64, dtype):
    """{tensor: largest |got - ref64| / (u_T M_e)}; elements whose magnitude is 0 must be exact."""
    out = {}
    for t in TENSORS:
        d = (got[t].double() - r64[t]).abs()
        m = r64["M_" + t] * U[dtype]
        pos = m > 0
        assert bool((d[~pos] == 0).all()), t
        out[t] = float((d[pos] / m[pos]).max()) if bool(pos.any()) else 0.0
    return out


def measure_constants(dtype):
    def build():
        worst = {t: 0.0 for t in TENSORS}
        for case in cases_for(dtype):
            inp = make_case(case, dtype)
            r = ratios(ref_T(inp), ref64(inp), dtype)
            worst = {t: max(worst[t], r[t]) for t in TENSORS}
        return worst
    return cached(("C", dtype), build)


def bound(r64, tensor, dtype, consts=None):
    C = (consts or C_MEASURED[dtype])[tensor]
    return 4.0 * C * U[dtype] * r64["M_" + tensor] + half_ulp(r64[tensor], dtype)


def lse_bound(r64):
    return 4.0 * U[F32] * (r64["lse"].abs() + r64["smax"]) + TRANS_F32 + half_ulp(r64["lse"], F32)


def check(got, r64, dtype, label, worst=None, consts=None):
    """Every element of every tensor in `got` against its bound; prints the worst |diff| / bound per tensor before it asserts. -> failures."""
    fails = []
    for t in got:
        b = lse_bound(r64) if t == "lse" else bound(r64, t, dtype, consts)
        d = (got[t].double().cpu() - r64[t]).abs()
        bad = ~(d <= b)
        pos = b > 0
        w = float((d[pos] / b[pos]).max()) if bool(pos.any()) else 0.0
        if worst is not None:
            worst[t] = max(worst.get(t, 0.0), w)
        print(f"{label} {t}: worst |diff| / bound {w:.4f}, {int(bad.sum())} of {bad.numel()} outside")
        if bool(bad.any()):
            fails.append((t, w, int(bad.sum())))
    return fails


# ------------------------------------------------------------------------------------------------ an independent f32 evaluation, with mistakes
MISTAKES = ("no_D", "dk_unscaled", "p_unnormalised", "ragged_key", "dv_drops_tile_last_query", "ds_is_dp", "dq_unscaled", "scale_twice_in_backward",
            "o_drops_last_key")


def applicable(mistake, N):
    if mistake == "ragged_key":
        return N % TILE != 0
    return True


def eval_f32(inp, mistake=None):
    """A flash-style evaluation in f32 (operands widened exactly; row maximum, lse, recomputed p), independent of ref64 and of the kernel."""
    q, k, v = inp["q"].float(), inp["k"].float(), inp["v"].float()
    heads, c, N = q.shape[1], inp["scale"], q.shape[2]
    do = _do_heads(inp["do"].float(), heads)
    kk, vv = k, v
    if mistake == "ragged_key":                                # the clamped load of key N taken for a real key
        kk, vv = torch.cat((k, k[:, :, -1:]), 2), torch.cat((v, v[:, :, -1:]), 2)
    s = (q @ kk.transpose(-1, -2)) * c
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    l = e.sum(-1, keepdim=True)
    ev = e.clone()
    if mistake == "o_drops_last_key":
        ev[..., -1] = 0
    o = (ev @ vv) / l
    lse = (m + torch.log(l))[..., 0]
    sb = s * c if mistake == "scale_twice_in_backward" else s
    p = torch.exp(sb - (m if mistake == "p_unnormalised" else lse[..., None]))
    D = (do * o).sum(-1, keepdim=True)
    dp = do @ vv.transpose(-1, -2)
    ds = p * dp if mistake == "no_D" else (dp if mistake == "ds_is_dp" else p * (dp - D))
    pv = p.clone()
    if mistake == "dv_drops_tile_last_query":
        pv[:, :, min(TILE, N) - 1] = 0
    dq = ds @ kk * (1.0 if mistake == "dq_unscaled" else c)
    dk = ds.transpose(-1, -2) @ q * (1.0 if mistake == "dk_unscaled" else c)
    dv = pv.transpose(-1, -2) @ do
    return dict(o=_merge(o), lse=lse, dq=dq, dk=dk[:, :, :N], dv=dv[:, :, :N])
