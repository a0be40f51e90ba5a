"""CPU: the ABI of the differentiable deformable cross-attention (csrc/msda_train.hip) and the bound of msda_train_ref.py.
  - the entry points are declared, exported and bound; the ctypes mirror of lwdetr_msda_train_desc has the compiler's layout;
  - every refusal of the header returns its code with made-up pointers and no device, and the launch record does not move;
  - the float64 restatement equals the recorded results of the unmodified reference module (tests/golden/msda_train.npz,
    tools/gen_golden_msda_train.py) within float64 round-off, and the explicit chain rule equals the restatement's autograd;
  - lwdetr_msda_train_backward_host - the kernels' own per-sample derivative and chain-rule functions, compiled for the host - is inside the
    bound on every case and dtype's inputs;
  - the restatement in float32 is inside the bound, and its worst ratios ARE the constants C[tensor] of msda_train_ref.C_MEASURED (measured
    again here, within [0.4, 1.5] x the table: a band and not equality, because another build of torch's CPU kernels may sum in another order);
  - each of eight mistakes planted in THIS MODULE'S explicit evaluation (msda_train_ref.evaluate - not in the kernels' code, which is covered by
    the host evaluation above and by the GPU tests) leaves the bound on the tensors that depend on it, on every case that can show it: the
    bound is tight enough to see each of them;
  - offsets / logits views that do not hold B Q rows (expanded, overlapping) are handed to the ABI as packed copies;
  - the Function, the module and the patch helper raise the documented error for host tensors.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import msda_train_helpers as MH
import msda_train_ref as R
from helpers import GOLDEN, ROOT

SYMBOLS = {"lwdetr_msda_train_forward": 3, "lwdetr_msda_train_workspace_bytes": 1, "lwdetr_msda_train_backward": 9,
           "lwdetr_msda_train_backward_host": 17, "lwdetr_msda_train_path_counts": 2, "lwdetr_msda_train_path_name": 1}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from lwdetr_amd import _native
    return _native


def test_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "lwdetr_hip.h")).read()
    declared = set(re.findall(r"\b(lwdetr_msda_train_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(SYMBOLS)
    raw = ctypes.CDLL(built.LIB_PATH)
    restype = {"lwdetr_msda_train_workspace_bytes": ctypes.c_long, "lwdetr_msda_train_path_name": ctypes.c_char_p}
    for sym, nargs in SYMBOLS.items():
        assert hasattr(raw, sym), f"{sym} declared in include/lwdetr_hip.h but not exported"
        fn = getattr(built.lib(), sym)
        assert len(fn.argtypes) == nargs and fn.restype is restype.get(sym, ctypes.c_int), sym
    names = list(built.msda_train_path_counts())
    assert len(names) == len(set(names)) == 27
    for dt in ("f32", "f16", "bf16"):
        assert all(f"msda_train_bwd_v_{dt}_e{e}" in names for e in (1, 2, 4))
        for form in ("l1p2", "l2p4", "gen"):
            assert f"msda_train_fwd_{dt}_{form}" in names and f"msda_train_bwd_q_{dt}_{form}" in names
    from lwdetr_amd import ops
    for name in ("FusedMSDeformAttnFunction", "MSDeformAttnTrain", "patch_deformable_attention", "MSDeformAttn", "MSDeformAttnFunction"):
        assert hasattr(ops, name)


def test_desc_mirror_has_the_compilers_layout(built, tmp_path):
    cls = built.MsdaTrainDesc
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lwdetr_hip.h"\nint main(){\nprintf("%zu", sizeof(lwdetr_msda_train_desc));\n'
           + "".join(f'printf(" %zu", offsetof(lwdetr_msda_train_desc, {f[0]}));\n' for f in cls._fields_) + 'printf("\\n");return 0;}\n')
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    ln = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    assert ln[0] == ctypes.sizeof(cls)
    assert ln[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]


def _desc(built, **kw):
    d = built.MsdaTrainDesc()
    base = dict(value=0x10000, value_ld=64, offsets=0x20000, offsets_ld=32, logits=0x30000, logits_ld=16, ref=0x40000, mask=None, shapes=0x50000,
                level_start=0x60000, B=2, S=30, M=4, D=16, L=1, Q=5, P=2, dtype=0)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_every_refusal_returns_its_code_without_a_device(built):
    """None of these reaches a launch: the pointers are made up."""
    l, BAD, UNS = built.lib(), built.ERR_BAD_ARG, built.ERR_UNSUPPORTED
    before = built.msda_train_path_counts()
    nrec = 2 * 4 * 1 * 5 * 2

    def fwd(out=0x70000, **kw):
        return l.lwdetr_msda_train_forward(_desc(built, **kw), out, None)

    def bwd(go=0x80000, gv=0x90000, goff=0xa0000, glg=0xb0000, gref=0xc0000, ws=0xd0000, ws_bytes=nrec * 20, **kw):
        return l.lwdetr_msda_train_backward(_desc(built, **kw), go, gv, goff, glg, gref, ws, ws_bytes, None)

    assert l.lwdetr_msda_train_forward(None, 0x70000, None) == BAD
    assert l.lwdetr_msda_train_backward(None, 1, 1, 1, 1, 1, 1, 1 << 20, None) == BAD
    assert l.lwdetr_msda_train_workspace_bytes(None) == 0
    for f in ("value", "offsets", "logits", "ref", "shapes", "level_start"):
        assert fwd(**{f: None}) == BAD and bwd(**{f: None}) == BAD, f
    assert fwd(out=None) == BAD
    for f in ("go", "gv", "goff", "glg", "gref", "ws"):
        assert bwd(**{f: None}) == BAD, f
    for f in ("B", "S", "M", "D", "L", "Q", "P"):
        assert fwd(**{f: 0}) == BAD and fwd(**{f: -3}) == BAD and bwd(**{f: 0}) == BAD, f
    for f, v in (("value_ld", 63), ("value_ld", 48), ("offsets_ld", 15), ("logits_ld", 7)):
        assert fwd(**{f: v}) == BAD and bwd(**{f: v}) == BAD, (f, v)
    assert fwd(value_ld=66) == BAD                                          # 264 bytes: rows leave the 16-byte grid
    assert fwd(dtype=2, value_ld=68) == BAD                                 # 136 bytes in bf16
    for f in ("value",):
        assert fwd(**{f: 0x10008}) == BAD and bwd(**{f: 0x10008}) == BAD, f
    assert fwd(out=0x70008) == BAD and bwd(go=0x80008) == BAD and bwd(ws=0xd0008) == BAD
    for f in ("offsets", "logits", "ref"):
        assert fwd(**{f: 0x20002}) == BAD, f                                # not aligned to a float
    assert fwd(dtype=1, offsets=0x20001) == BAD and fwd(shapes=0x50004) == BAD and fwd(level_start=0x60004) == BAD
    for f in ("gv", "goff", "glg", "gref"):
        assert bwd(**{f: 0x90002}) == BAD, f
    assert bwd(ws_bytes=nrec * 20 - 1) == BAD and bwd(ws_bytes=0) == BAD
    for kw in (dict(D=12), dict(D=4), dict(D=72, value_ld=4 * 72), dict(L=5), dict(P=3), dict(P=16), dict(L=4, P=8), dict(L=3, P=8), dict(M=257, value_ld=257 * 16),
               dict(dtype=3), dict(dtype=-1), dict(dtype=7)):
        assert fwd(**kw) == UNS and bwd(**kw) == UNS, kw
        assert l.lwdetr_msda_train_workspace_bytes(_desc(built, **kw)) == 0
    assert fwd(dtype=3, value=None) == UNS                                  # the range is judged before the pointers
    assert built.msda_train_path_counts() == before
    assert l.lwdetr_msda_train_workspace_bytes(_desc(built)) == nrec * 20
    assert l.lwdetr_msda_train_workspace_bytes(_desc(built, B=4, M=24, L=2, Q=3900, P=4, logits_ld=192, offsets_ld=384, value_ld=384)) == 4 * 24 * 2 * 3900 * 4 * 20
    z = (ctypes.c_float * 64)()
    zi = (ctypes.c_int64 * 8)()
    p = lambda a: ctypes.cast(a, ctypes.c_void_p)
    host = l.lwdetr_msda_train_backward_host
    assert host(None, 8, None, p(zi), p(zi), 8, 1, 1, p(z), p(z), p(z), p(z), p(z), 8, p(z), p(z), p(z)) == BAD
    assert host(p(z), 4, None, p(zi), p(zi), 8, 1, 1, p(z), p(z), p(z), p(z), p(z), 8, p(z), p(z), p(z)) == BAD
    assert host(p(z), 8, None, p(zi), p(zi), 8, 3, 8, p(z), p(z), p(z), p(z), p(z), 8, p(z), p(z), p(z)) == UNS


def test_python_layer_raises_for_host_tensors(built):
    from lwdetr_amd import ops
    shapes, lsi = torch.tensor([[3, 5]]), torch.tensor([0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.FusedMSDeformAttnFunction.apply(torch.zeros(1, 15, 2, 8), shapes, lsi, torch.zeros(1, 4, 8), torch.zeros(1, 4, 4), torch.zeros(1, 4, 1, 4))
    m = ops.MSDeformAttnTrain(32, 1, 2, 2)
    assert sorted(m.state_dict()) == sorted(ops.MSDeformAttn(32, 1, 2, 2).state_dict())
    for (k, a), (_, b) in zip(sorted(m.state_dict().items()), sorted(ops.MSDeformAttn(32, 1, 2, 2).state_dict().items())):
        assert a.shape == b.shape, k
        if "value_proj.weight" not in k and "output_proj.weight" not in k:      # those two are drawn at random
            assert torch.equal(a, b), k
    args = (torch.zeros(1, 4, 32), torch.zeros(1, 4, 1, 4), torch.zeros(1, 15, 32), shapes, lsi)
    with pytest.raises(RuntimeError, match="ROCm device"):
        m(*args)

    class StandIn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.n_heads, self.n_levels, self.n_points = 2, 1, 2
            self.sampling_offsets, self.attention_weights = torch.nn.Linear(32, 8), torch.nn.Linear(32, 4)
            self.value_proj, self.output_proj = torch.nn.Linear(32, 32), torch.nn.Linear(32, 32)

    model = torch.nn.Sequential(StandIn(), torch.nn.Linear(4, 4), StandIn())
    keys = sorted(model.state_dict())
    assert ops.patch_deformable_attention(model) == 2 and sorted(model.state_dict()) == keys
    with pytest.raises(RuntimeError, match="ROCm device"):
        model[0](*args)


# -------------------------------------------------------------------------------------------------------------------- the restatement
def test_restatement_equals_the_recorded_reference_module():
    """float64 against float64: 1e-12 of the element's magnitude (the reference samples with grid_sample, whose weights are formed from
    2 loc - 1; the two differ by a few float64 roundings of the coordinate). grad_ref of the rows that sit exactly on the border of the map
    is left out: grid_sample has a one-sided derivative there, the operator's strict rule has none (tools/gen_golden_msda_train.py)."""
    g = np.load(os.path.join(GOLDEN, "msda_train.npz"), allow_pickle=False)
    for name in R.GOLDEN_CASES:
        case = next(c for c in R.CASES if c["name"] == name)
        inp = R.make_case(case, R.F32)
        r64 = R.ref64(inp)
        for t in R.TENSORS:
            idx = torch.from_numpy(g[f"{name}/{t}/index"])
            want = torch.from_numpy(g[f"{name}/{t}/value"])
            have, mag = r64[t].reshape(-1)[idx], r64["M_" + t].reshape(-1)[idx]
            keep = torch.ones_like(idx, dtype=torch.bool)
            if t == "grad_ref":
                keep = ~inp["engineered"][:, :, None, None].expand_as(r64[t]).reshape(-1)[idx]
            d = (have - want).abs()
            if not bool(keep.any()):                                            # Q = 3: every row is an engineered one
                continue
            print(f"{name} {t}: {int(keep.sum())} recorded elements, worst |restatement - reference| / M_e {float((d / mag.clamp_min(1e-300))[keep].max()):.2e}; "
                  f"reference f32 distance {float(g[f'{name}/{t}/f32_distance']):.2f}")
            assert bool((d <= 1e-12 * mag + 1e-300)[keep].all()), (name, t)
            assert float(g[f"{name}/{t}/f32_distance"]) <= 1.5 * R.C_MEASURED[t], (name, t)


def test_explicit_chain_rule_equals_autograd_in_float64():
    for case in R.CASES:
        inp = R.make_case(case, R.BF16)
        r64, ev = R.ref64(inp), R.evaluate(inp, torch.float64)
        for t in R.TENSORS:
            assert bool(((ev[t].reshape(r64[t].shape) - r64[t]).abs() <= 1e-12 * r64["M_" + t] + 1e-300).all()), (case["name"], t)


def test_float32_restatement_is_inside_the_bound_and_gives_the_constants():
    for dtype in R.DTYPES:
        for case in R.ALL_CASES:                             # the near-edge case under its own bound; C comes from R.CASES alone
            inp = R.make_case(case, dtype)
            fails = R.check(R.restate(inp, torch.float32), R.ref64(inp), R.F32, f"{case['name']} {R.NAME[dtype]} inputs, f32 restatement")
            assert not fails, (case["name"], fails)
    measured = R.measure_constants()
    print("measured C:", {t: round(c, 2) for t, c in measured.items()}, "table:", R.C_MEASURED)
    for t in R.TENSORS:
        assert 0.4 * R.C_MEASURED[t] <= measured[t] <= 1.5 * R.C_MEASURED[t], (t, measured[t])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
def test_host_evaluation_is_inside_the_bound(built, dtype):
    """The kernels' own derivative and chain-rule functions on the host, in f32 on the inputs of every dtype: the f32 bound."""
    for case in R.ALL_CASES:
        inp = R.make_case(case, dtype)
        fails = R.check(MH.host_backward(built, inp), R.ref64(inp), R.F32, f"{case['name']} {R.NAME[dtype]} inputs, host evaluation")
        assert not fails, (case["name"], fails)


def test_explicit_f32_evaluation_is_inside_the_bound():
    for case in R.ALL_CASES:
        inp = R.make_case(case, R.F32)
        assert not R.check(R.evaluate(inp, torch.float32), R.ref64(inp), R.F32, f"{case['name']} explicit f32 evaluation")


@pytest.mark.parametrize("mistake", list(R.MISTAKES))
def test_each_planted_mistake_leaves_the_bound(mistake):
    """Sensitivity of the bound: the mistake is made in msda_train_ref.evaluate (torch, f32), not in the code under test."""
    deps, applies = R.MISTAKES[mistake]
    hit = 0
    for case in R.CASES:
        if not applies(case):
            continue
        inp = R.make_case(case, R.F32)
        fails = {t for t, _, _ in R.check(R.evaluate(inp, torch.float32, mistake=mistake), R.ref64(inp), R.F32, f"{case['name']} {mistake}")}
        assert set(deps) <= fails, f"{mistake} stays inside the bound on {case['name']}: outside {sorted(fails)}, expected {deps}"
        hit += 1
    assert hit >= 3


def test_row_views_that_do_not_hold_their_rows_are_copied():
    """The ABI reads row r of offsets / logits at r * ld: a view whose row stride is 0 (expand) or below the width (overlapping as_strided)
    must not be passed with a made-up ld."""
    from lwdetr_amd.ops import deform_train as T
    for t in (torch.zeros(1, 1, 8).expand(1, 5, 8), torch.zeros(2, 1, 8).expand(2, 5, 8), torch.as_strided(torch.zeros(64), (1, 5, 8), (0, 3, 1)),
              torch.as_strided(torch.zeros(64), (2, 1, 8), (4, 8, 1)), torch.zeros(1, 5, 2, 2, 2).expand(3, 5, 2, 2, 2)):
        r, ld = T._rows(t, t.shape[0] * t.shape[1], 8)
        assert ld == 8 and r.is_contiguous() and r.untyped_storage().nbytes() >= t.shape[0] * t.shape[1] * 8 * 4, t.stride()
    wide = torch.zeros(2, 5, 24)
    r, ld = T._rows(wide[:, :, 8:16], 10, 8)                # a column view of a Linear's output stays a view
    assert ld == 24 and r.data_ptr() == wide[:, :, 8:16].data_ptr()
    r, ld = T._rows(wide[:, :1, 8:16], 2, 8)
    assert ld == 120 and r.data_ptr() == wide[:, :1, 8:16].data_ptr()


def test_near_edge_case_needs_its_coordinate_term_and_still_sees_mistakes():
    """Without E_e the float32 restatement itself leaves the bound on the near-edge case (that is why the other cases keep 2^-5), with it the
    planted mistakes still do."""
    for case in R.NEAR_EDGE_CASES:
        inp = R.make_case(case, R.F32)
        r64 = R.ref64(inp)
        bare = {k: v for k, v in r64.items() if not k.startswith("E_")}
        assert R.check(R.restate(inp, torch.float32), bare, R.F32, f"{case['name']} without the coordinate term")
        for mistake in ("off_no_P", "no_half", "softmax_no_dot", "lh_hh_swapped"):
            fails = {t for t, _, _ in R.check(R.evaluate(inp, torch.float32, mistake=mistake), r64, R.F32, f"{case['name']} {mistake}")}
            assert set(R.MISTAKES[mistake][0]) <= fails, (mistake, sorted(fails))
