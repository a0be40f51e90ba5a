"""CPU: the ABI of the differentiable fused attention (csrc/attention_train.hip) and the bound of attn_train_ref.py.
  - the entry points are declared, exported and bound; the ctypes mirror of lwdetr_attn_train_desc has the compiler's layout;
  - every refusal of the header returns its code with no device present, and the Python layer raises for CPU tensors;
  - the reference formulation in f32 / f16 / bf16 stays inside the bound on every case, and its worst ratios ARE the constants C[T][tensor] of
    attn_train_ref.C_MEASURED (measured again here, within [0.4, 1.5] x the table - a band and not equality because another build of
    torch's CPU matmul may sum in another order; 1, 4 and 8 threads gave the table's figures to every digit);
  - an independent f32 evaluation stays inside the bound, and each of nine planted mistakes leaves it on every case it applies to.
"""
import ctypes
import os
import re
import subprocess

import pytest
import torch

import attn_train_ref as R
from helpers import ROOT

SYMBOLS = {"lwdetr_attn_train_forward": 3, "lwdetr_attn_train_workspace_bytes": 5, "lwdetr_attn_train_backward": 18,
           "lwdetr_attn_train_path_counts": 2, "lwdetr_attn_train_path_name": 1}


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from lwdetr_amd import _native
    return _native


def test_symbols_are_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "lwdetr_hip.h")).read()
    declared = set(re.findall(r"\b(lwdetr_attn_train_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(SYMBOLS)
    raw = ctypes.CDLL(built.LIB_PATH)
    restype = {"lwdetr_attn_train_workspace_bytes": ctypes.c_long, "lwdetr_attn_train_path_name": ctypes.c_char_p}
    for sym, nargs in SYMBOLS.items():
        assert hasattr(raw, sym), f"{sym} declared in include/lwdetr_hip.h but not exported"
        fn = getattr(built.lib(), sym)
        assert len(fn.argtypes) == nargs and fn.restype is restype.get(sym, ctypes.c_int), sym
    names = list(built.attn_train_path_counts())
    assert len(names) == len(set(names)) == 39
    for dt in ("f32", "f16", "bf16"):
        assert f"attn_train_bwd_dot_{dt}" in names
        for hd in (16, 32, 64):
            for form in ("fwd", "bwd_one", "bwd_dkdv", "bwd_dq"):
                assert f"attn_train_{form}_{dt}_hd{hd}" in names
    from lwdetr_amd import ops
    for name in ("Attention", "FusedAttentionFunction", "fused_attention", "patch_vit_attention"):
        assert hasattr(ops, name)


def test_desc_mirror_has_the_compilers_layout(built, tmp_path):
    cls = built.AttnTrainDesc
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lwdetr_hip.h"\nint main(){\nprintf("%zu", sizeof(lwdetr_attn_train_desc));\n'
           + "".join(f'printf(" %zu", offsetof(lwdetr_attn_train_desc, {f[0]}));\n' for f in cls._fields_) + 'printf("\\n");return 0;}\n')
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    ln = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    assert ln[0] == ctypes.sizeof(cls)
    assert ln[1:] == [getattr(cls, f[0]).offset for f in cls._fields_]


def _desc(built, **kw):
    d = built.AttnTrainDesc()
    base = dict(q=0x1000, k=0x2000, v=0x3000, o=0x4000, lse=0x5000, q_sb=4096, q_sn=96, q_sh=16, k_sb=4096, k_sn=96, k_sh=16, v_sb=4096, v_sn=96,
                v_sh=16, o_ld=32, B=1, heads=2, N=8, hd=16, scale=0.25)
    base.update(kw)
    for k, v in base.items():
        setattr(d, k, v)
    return d


def test_every_refusal_returns_its_code_without_a_device(built):
    """None of these reaches a launch: the pointers are made up."""
    l, BAD, UNS = built.lib(), built.ERR_BAD_ARG, built.ERR_UNSUPPORTED
    before = built.attn_train_path_counts()
    gs = [4096, 96, 16] * 3

    def fwd(dtype=0, **kw):
        return l.lwdetr_attn_train_forward(_desc(built, **kw), dtype, None)

    def bwd(dtype=0, d_o=0x6000, do_ld=32, dq=0x7000, dk=0x8000, dv=0x9000, strides=gs, ws=None, **kw):
        return l.lwdetr_attn_train_backward(_desc(built, **kw), d_o, do_ld, dq, dk, dv, *strides, ws, dtype, None)

    assert l.lwdetr_attn_train_forward(None, 0, None) == BAD
    for f in ("q", "k", "v", "o", "lse"):
        assert fwd(**{f: None}) == BAD and bwd(**{f: None}) == BAD, f
    for f in ("d_o", "dq", "dk", "dv"):
        assert bwd(**{f: None}) == BAD, f
    for f in ("B", "heads", "N"):
        assert fwd(**{f: 0}) == BAD and fwd(**{f: -3}) == BAD and bwd(**{f: 0}) == BAD, f
    for s in (0.0, -0.25, float("nan"), float("inf")):
        assert fwd(scale=s) == BAD and bwd(scale=s) == BAD, s
    for f in ("q", "k", "v", "o"):
        assert fwd(**{f: 0x1008}) == BAD and bwd(**{f: 0x1008}) == BAD, f
    for f in ("d_o", "dq", "dk", "dv"):
        assert bwd(**{f: 0x7008}) == BAD, f
    for f in ("q_sb", "q_sn", "q_sh", "k_sb", "k_sn", "k_sh", "v_sb", "v_sn", "v_sh", "o_ld"):
        assert fwd(**{f: 18}) == BAD, f                                     # 72 bytes in f32
        assert fwd(dtype=2, **{f: 20}) == BAD, f                            # 40 bytes in bf16
    assert bwd(do_ld=34) == BAD
    for i in range(9):
        assert bwd(strides=gs[:i] + [gs[i] + 2] + gs[i + 1:]) == BAD, i
    assert bwd(N=300, ws=None) == BAD                                       # the long form needs its workspace
    for hd in (0, 8, 24, 48, 128):
        assert fwd(hd=hd) == UNS and bwd(hd=hd) == UNS, hd
    for dtype in (-1, 3, 7):
        assert fwd(dtype=dtype) == UNS and bwd(dtype=dtype) == UNS, dtype
    assert built.attn_train_path_counts() == before
    assert l.lwdetr_attn_train_workspace_bytes(4, 12, 100, 16, 0) == 0
    assert l.lwdetr_attn_train_workspace_bytes(4, 12, 256, 16, 0) == 0
    assert l.lwdetr_attn_train_workspace_bytes(4, 12, 257, 16, 2) == 4 * 12 * 257 * 4
    assert l.lwdetr_attn_train_workspace_bytes(1, 12, 3136, 64, 1) == 12 * 3136 * 4


def test_python_layer_raises_for_cpu_tensors(built):
    from lwdetr_amd import ops
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.FusedAttentionFunction.apply(torch.zeros(1, 8, 3, 2, 16), 0.25)
    q = torch.zeros(1, 2, 8, 16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.fused_attention(q, q, q, 0.25)
    m = ops.Attention(64, 4)
    assert sorted(m.state_dict()) == ["proj.bias", "proj.weight", "qkv.bias", "qkv.weight"]
    assert sorted(ops.Attention(64, 4, use_cae=True).state_dict()) == ["proj.bias", "proj.weight", "q_bias", "qkv.weight", "v_bias"]
    assert ops.patch_vit_attention(torch.nn.Sequential(m, torch.nn.Linear(4, 4))) == 1


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.NAME[d])
def test_reference_formulation_is_inside_the_bound_and_gives_the_constants(dtype):
    worst = {}
    for case in R.cases_for(dtype):
        inp = R.make_case(case, dtype)
        fails = R.check(R.ref_T(inp), R.ref64(inp), dtype, f"{case['name']} {R.NAME[dtype]} reference formulation", worst)
        assert not fails, (case["name"], fails)
    measured = R.measure_constants(dtype)
    print(R.NAME[dtype], "measured C:", {t: round(c, 4) for t, c in measured.items()}, "table:", R.C_MEASURED[dtype])
    for t in R.TENSORS:
        assert 0.4 * R.C_MEASURED[dtype][t] <= measured[t] <= 1.5 * R.C_MEASURED[dtype][t], (t, measured[t])


PLANT_CASES = [c for c in R.CASES if 17 <= c["N"] <= 300]


def test_independent_f32_evaluation_is_inside_the_bound():
    for case in R.cases_for(R.F32):
        if case["N"] > 800:
            continue
        inp = R.make_case(case, R.F32)
        assert not R.check(R.eval_f32(inp), R.ref64(inp), R.F32, f"{case['name']} f32 evaluation")


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_each_planted_mistake_leaves_the_bound(mistake):
    hit = 0
    for case in PLANT_CASES:
        if not R.applicable(mistake, case["N"]):
            continue
        inp = R.make_case(case, R.F32)
        fails = R.check(R.eval_f32(inp, mistake), R.ref64(inp), R.F32, f"{case['name']} {mistake}")
        assert fails, f"{mistake} stays inside the bound on {case['name']}"
        hit += 1
    assert hit >= 5
