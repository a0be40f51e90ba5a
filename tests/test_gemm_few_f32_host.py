"""CPU: the host side of the float32 form of lwdetr_gemm_few (lw-detr_amd/csrc/few.hip).

(1) A lane-level numpy emulation of the kernel's f32 fragment loads and of Mma<float>::k32 (eight 16x16x4 MFMAs per chunk of 32) on
    kernels.pack_frag16(W): lane (l15, g) holds k = 32 c + 8 g + s of its row for BOTH operands, slice s contracts over { 32 c + 8 g' + s }.
(2) kernels.few_entry_takes(d, torch.float32) against a table of descriptors, one per refusal of the C entry; the plan switch LWDETR_GEMM_FEW_F32.
(3) tools/kernel_regs.py on the built library: no f32 instantiation of gemm_few_kernel spills or uses scratch (metadata only, no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- (1) lane-level emulation
def _mfma_16x16x4(a_lane, b_lane, acc):
    """v_mfma_f32_16x16x4_f32 (common.h): A operand lane l = A[i = l & 15][k = l >> 4], B operand lane l = B[k = l >> 4][j = l & 15],
    D lane l, register r = D[i = 4 (l >> 4) + r][j = l & 15]. a_lane, b_lane: (64,), acc: (64, 4)."""
    Am = np.zeros((16, 4)); Bm = np.zeros((4, 16))
    for l in range(64):
        Am[l & 15, l >> 4] = a_lane[l]
        Bm[l >> 4, l & 15] = b_lane[l]
    D = Am @ Bm
    out = acc.copy()
    for l in range(64):
        for r in range(4):
            out[l, r] += D[4 * (l >> 4) + r, l & 15]
    return out


def _emulate_few_f32(A, Wf, x_k=None):
    """out (M = 16, N) of one 16-row workgroup: wave n_tile loads, per chunk c, wa = Wf[n_tile][c][l15][8 g .. 8 g + 7] (one contiguous fragment)
    and xa = A[row l15][k(c, g, s)], s = 0..7 - k(c, g, s) = 32 c + 8 g + s in the kernel - and issues k32(wa, xa, acc): W is the A operand."""
    x_k = x_k or (lambda c, g, s: 32 * c + 8 * g + s)
    ntile, nchunks = Wf.shape[0], Wf.shape[1]
    out = np.zeros((16, 16 * ntile))
    for n_tile in range(ntile):
        acc = np.zeros((64, 4))
        for c in range(nchunks):
            wa = np.stack([Wf[n_tile, c, l & 15, 8 * (l >> 4):8 * (l >> 4) + 8] for l in range(64)])           # (64, 8)
            xa = np.stack([[A[l & 15, x_k(c, l >> 4, s)] for s in range(8)] for l in range(64)])
            for s in range(8):
                acc = _mfma_16x16x4(wa[:, s], xa[:, s], acc)
        for l in range(64):                                          # epilogue: lane (row l15, g) holds columns 4 g .. 4 g + 3
            out[l & 15, 16 * n_tile + 4 * (l >> 4):16 * n_tile + 4 * (l >> 4) + 4] = acc[l]
    return out


def test_f32_fragment_lanes_reproduce_the_product_exactly():
    from lwdetr_amd import kernels as K
    g = torch.Generator().manual_seed(3)
    A = torch.randint(-7, 8, (16, 64), generator=g).double()         # small integers: every order of the sum is exact
    W = torch.randint(-7, 8, (32, 64), generator=g).double()
    Wf = K.pack_frag16(W)
    assert tuple(Wf.shape) == (2, 2, 16, 32) and Wf.is_contiguous()
    assert Wf[0, 0].numel() * 4 == 2048                              # an f32 fragment is one contiguous 2 KB
    ref = (A @ W.t()).numpy()
    got = _emulate_few_f32(A.numpy(), Wf.numpy())
    assert np.array_equal(got, ref)
    # the slice permutation on ONE operand only (x in the natural order of 16x16x4, k = 4 s + g inside each run of 32; W as packed): wrong
    bad = _emulate_few_f32(A.numpy(), Wf.numpy(), x_k=lambda c, g_, s: 32 * c + 4 * s + g_ if s < 4 else 32 * c + 16 + 4 * (s - 4) + g_)
    assert not np.array_equal(bad, ref)
    assert np.abs(bad - ref).max() > 1


# ---------------------------------------------------------------------------------------------------------------- (2) the Python predicates
def _desc(**kw):
    """A descriptor lwdetr_gemm_few takes in f32 AND in 16-bit (every pointer 32-byte aligned, lda % 8): M = 64, N = 32, K = 64, ldo = 48."""
    from lwdetr_amd._native import GemmDesc
    d = GemmDesc()
    d.A, d.W, d.M, d.N, d.K, d.lda, d.nseg = 0x10000, 0x20000, 64, 32, 64, 64, 1
    s = d.seg[0]
    s.out, s.ldo, s.n_begin, s.n_end, s.scale = 0x30000, 48, 0, 32, 1.0
    s.bias, s.gamma, s.res, s.ldres, s.out2, s.ld2 = 0x40000, 0x50000, 0x60000, 48, 0x70000, 48
    for k, v in kw.items():
        setattr(d if hasattr(d, k) else s, k, v)
    return d


# what the C entry refuses (few.hip, lwdetr_gemm_few), one descriptor each
F32_REFUSED = {
    "row mask": dict(rowmask=0x80000),
    "N % 16": dict(N=24, n_end=24),
    "n_end > N": dict(n_end=48),
    "n_end < N": dict(n_end=16),
    "K = 48": dict(K=48),
    "res at an 8-byte offset": dict(res=0x60008),
    "out2 at an 8-byte offset": dict(out2=0x70008),
    "out at an 8-byte offset": dict(out=0x30008),
    "bias at an 8-byte offset": dict(bias=0x40008),
    "gamma at an 8-byte offset": dict(gamma=0x50008),
    "lda % 4": dict(lda=66),
    "ldo % 4": dict(ldo=50),
    "ldres % 4": dict(ldres=50),
    "ld2 % 4": dict(ld2=50),
    "A at an 8-byte offset": dict(A=0x10008),
    "W at an 8-byte offset": dict(W=0x20008),
    "ln_stats": dict(ln_stats=0x90000),
    "res_mod": dict(res_mod=16),
    "A2": dict(A2=0xA0000),
    "HEADS mode": dict(mode=1),
    "two segments": dict(nseg=2),
    "n_begin": dict(n_begin=16),
    "M > 8192": dict(M=8193),
    "unknown activation": dict(act=4),
    "negative activation": dict(act=-1),
    "CONV a_mode (the predicate is about PLAIN A)": dict(a_mode=1),
}


def test_few_entry_takes_accepts_the_base_descriptor():
    from lwdetr_amd import kernels as K
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert K.few_entry_takes(_desc(), dt)
    assert not K.few_entry_takes(_desc(), torch.float64)
    # no optional operand at all
    assert K.few_entry_takes(_desc(bias=None, gamma=None, res=None, out2=None), torch.float32)


@pytest.mark.parametrize("what", list(F32_REFUSED))
def test_few_entry_takes_f32_mirrors_each_refusal(what):
    from lwdetr_amd import kernels as K
    assert not K.few_entry_takes(_desc(**F32_REFUSED[what]), torch.float32), what


def test_few_entry_takes_alignment_rules_differ_by_dtype():
    """f32: runs of 4 values are 16 bytes (out / res / out2 16-byte aligned), A rows in 16-byte loads of 4 (lda % 4); 16-bit: 8 bytes, lda % 8."""
    from lwdetr_amd import kernels as K
    for field, ptr in (("out", 0x30008), ("res", 0x60008), ("out2", 0x70008)):
        d = _desc(**{field: ptr})
        assert K.few_entry_takes(d, torch.float16) and K.few_entry_takes(d, torch.bfloat16) and not K.few_entry_takes(d, torch.float32), field
        d = _desc(**{field: ptr - 4})                                # 4-byte offset: nobody takes it
        assert not K.few_entry_takes(d, torch.float16) and not K.few_entry_takes(d, torch.float32), field
    d = _desc(lda=68)
    assert K.few_entry_takes(d, torch.float32) and not K.few_entry_takes(d, torch.float16)
    d = _desc(lda=72)
    assert K.few_entry_takes(d, torch.float32) and K.few_entry_takes(d, torch.float16)


def test_gemm_few_supported_takes_f32_only_behind_its_switch(monkeypatch):
    from lwdetr_amd import kernels as K
    F32, F16 = torch.float32, torch.float16
    monkeypatch.delenv("LWDETR_GEMM_FEW", raising=False)
    monkeypatch.delenv("LWDETR_GEMM_FEW_F32", raising=False)
    shapes = [(1600, K.A_CONV3x3, 128, 1152), (3200, K.A_CONV3x3, 192, 1728), (300, K.A_PLAIN, 0, 256), (640, K.A_PLAIN, 0, 512)]
    for m, am, cin, k in shapes:
        assert not K.gemm_few_supported(F32, m, am, cin, k)          # the default: off
        assert K.gemm_few_supported(F16, m, am, cin, k)
    monkeypatch.setenv("LWDETR_GEMM_FEW_F32", "0")
    assert not any(K.gemm_few_supported(F32, m, am, cin, k) for m, am, cin, k in shapes)
    monkeypatch.setenv("LWDETR_GEMM_FEW_F32", "1")
    for m, am, cin, k in shapes:
        assert K.gemm_few_supported(F32, m, am, cin, k)
    # ... under the shape rules of 16-bit
    for dt in (F32, F16):
        assert not K.gemm_few_supported(dt, K.GEMM_FEW_MAX_ROWS + 1, K.A_CONV3x3, 128, 1152)
        assert not K.gemm_few_supported(dt, 1600, K.A_CONV3x3, 64, 576)
        assert not K.gemm_few_supported(dt, 300, K.A_PLAIN, 0, 224)
        assert not K.gemm_few_supported(dt, 641, K.A_PLAIN, 0, 256)
        assert not K.gemm_few_supported(dt, 300, K.A_PATCH16, 0, 768)
    assert not K.gemm_few_supported(torch.float64, 300, K.A_PLAIN, 0, 256)
    monkeypatch.setenv("LWDETR_GEMM_FEW", "2")
    assert K.gemm_few_supported(F32, 1600, K.A_PLAIN, 0, 256) and K.gemm_few_supported(F16, 1600, K.A_PLAIN, 0, 256)
    monkeypatch.setenv("LWDETR_GEMM_FEW", "0")
    for m, am, cin, k in shapes:
        assert not K.gemm_few_supported(F32, m, am, cin, k) and not K.gemm_few_supported(F16, m, am, cin, k)
    monkeypatch.setenv("LWDETR_GEMM_FEW", "1")
    monkeypatch.delenv("LWDETR_GEMM_FEW_F32")
    assert K.gemm_few_supported(F16, 1600, K.A_CONV3x3, 128, 1152) and not K.gemm_few_supported(F32, 1600, K.A_CONV3x3, 128, 1152)


# ---------------------------------------------------------------------------------------------------------------- (3) registers of the build
def test_f32_few_row_kernels_use_no_scratch():
    """Every gemm_few_kernel<float, ...> of the built library: no scratch, no spilled registers, within the 256 registers that
    __launch_bounds__(512) leaves a wave; PLAIN, CONV Cin = 128 (KCH 4) and CONV Cin = 192 (KCH 6) are all there."""
    from lwdetr_amd import _native
    assert _native.is_built(), f"{_native.LIB_PATH} is not built"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    rows = [r for r in kernel_regs.kernel_table(_native.LIB_PATH) if "gemm_few_kernelIf" in r["symbol"]]      # Itanium mangling: If = <float
    forms = sorted(r["symbol"].split("gemm_few_kernelIf")[1][:8] for r in rows)
    assert [f[:8] for f in forms] == ["Li0ELi4E", "Li1ELi4E", "Li1ELi6E"], [r["symbol"] for r in rows]      # (AMODE, KCH)
    for r in rows:
        assert r["private_segment_fixed_size"] == 0, r
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["vgpr_count"] is not None and r["vgpr_count"] <= 256, r
        assert r["group_segment_fixed_size"] == 0, r                 # no LDS
    # the 16-bit instantiations are found by the same walk (the filter above is not vacuous)
    assert len([r for r in kernel_regs.kernel_table(_native.LIB_PATH) if "gemm_few_kernelID" in r["symbol"]]) == 6
