"""CPU: the host side of the float32 form of lwdetr_vit_block_few (mlp_small_kernel<float, QKV, 1, true>, lw-detr_amd/csrc/mlp.hip).

(1) A lane-level numpy emulation of the f32 data flow of one 16-token workgroup on small integers (every order of every sum is exact):
    projection accumulators -> x1 rows in LDS -> B fragments in k-slot order -> fc1 on pack_frag16(pack_mlp_weights(proj=True)) -> the hidden fragment
    built from the two accumulators -> fc2 on the chunk-major w2c -> the new rows in LDS -> QKV on pack_frag16(pack_qkv_weights), V^T with the operands
    swapped. Mma<float>::k32 is eight 16x16x4 MFMAs; slice s pairs slot 8 g + s of both operands. The result equals the plain matrix formulation exactly:
    the packers of the 16-bit kernel serve float32 unchanged. (LayerNorm and GELU act per element / per row between the products and are left out: identity
    affine, no activation.)
(2) kernels.vit_block_few_entry_takes against one argument set per f32 refusal of the C entry; the plan switch LWDETR_VIT_BLOCK_FEW_F32.
(3) tools/kernel_regs.py on the built library: no mlp_small_kernel<float, ...> spills or uses scratch (metadata only, no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

from test_gemm_few_f32_host import _mfma_16x16x4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, KC, NT, HID = 192, 6, 12, 768
L15 = np.arange(64) & 15
G = np.arange(64) >> 4


# ---------------------------------------------------------------------------------------------------------------- (1) lane-level emulation
def _k32(a, b, acc):
    """Mma<float>::k32 (common.h): a, b (64 lanes, 8 values), acc (64, 4); a is the A operand."""
    for s in range(8):
        acc = _mfma_16x16x4(a[:, s], b[:, s], acc)
    return acc


def _wfrag(wf, rt, kc):
    """A weight fragment as the kernel loads it: lane (l15, g) reads 8 consecutive values at l15 * 32 + g * 8 of the contiguous 16 x 32 block."""
    blk = wf[rt, kc].reshape(-1)
    return np.stack([blk[l15 * 32 + g * 8:l15 * 32 + g * 8 + 8] for l15, g in zip(L15, G)])


def _rows_as_bfrag(rows, kc, k_of=None):
    """Rows [16][C] in LDS -> the B fragment of k-chunk kc: lane (token l15, g), slot h * 4 + e <- channel 32 kc + 16 h + 4 g + e."""
    k_of = k_of or (lambda g, h, e: 16 * h + 4 * g + e)
    return np.stack([[rows[l15, 32 * kc + k_of(g, h, e)] for h in range(2) for e in range(4)] for l15, g in zip(L15, G)])


def _emulate_block(x, att, wpf, bp, w1f, b1, w2c, b2, wqf, bq, k_of=None):
    """One workgroup (16 tokens) of mlp_small_f32 without LayerNorm / GELU / LayerScale: (new rows [16][C], q / k as [token][feature], v^T tile-wise
    as [token][feature] too - written from the swapped-operand accumulator layout)."""
    x1s = np.zeros((16, C))
    for pc in range(KC):                                             # projection: waves 0-5
        af = [np.stack([att[l15, 32 * kc + 8 * g:32 * kc + 8 * g + 8] for l15, g in zip(L15, G)]) for kc in range(KC)]
        for h in range(2):
            acc = np.zeros((64, 4))
            for kc in range(KC):
                acc = _k32(_wfrag(wpf, pc * 2 + h, kc), af[kc], acc)
            for l in range(64):                                      # accumulator lane (token l15, g): channels 4 g .. 4 g + 3 of the tile
                c0 = pc * 32 + h * 16 + 4 * G[l]
                x1s[L15[l], c0:c0 + 4] = x[L15[l], c0:c0 + 4] + acc[l] + bp[c0:c0 + 4]
    xf = [_rows_as_bfrag(x1s, kc, k_of) for kc in range(KC)]
    acc2 = [np.zeros((64, 4)) for _ in range(NT)]
    for hc in range(HID // 32):                                      # every wave's chunks; the cross-wave reduction is a plain sum
        acc1 = []
        for h in range(2):
            a = np.stack([b1[hc * 32 + 16 * h + 4 * g:hc * 32 + 16 * h + 4 * g + 4] for g in G]).astype(np.float64)
            for kc in range(KC):
                a = _k32(_wfrag(w1f, hc * 2 + h, kc), xf[kc], a)
            acc1.append(a)
        hf = np.concatenate([acc1[0], acc1[1]], axis=1)              # slots 0-3 <- tile 0, 4-7 <- tile 1
        for n in range(NT):
            w = np.stack([w2c[hc, n * 16 + l15, 8 * g:8 * g + 8] for l15, g in zip(L15, G)])
            acc2[n] = _k32(w, hf, acc2[n])
    for n in range(NT):
        for l in range(64):
            c0 = n * 16 + 4 * G[l]
            x1s[L15[l], c0:c0 + 4] += acc2[n][l] + b2[c0:c0 + 4]
    out = x1s.copy()
    xq = [_rows_as_bfrag(x1s, kc, k_of) for kc in range(KC)]
    qkv = np.zeros((16, 3 * C))
    for nt in range(3 * C // 16):
        sg = nt // NT
        if sg < 2:                                                   # D[feature 4 g + r][token l15]
            acc = np.stack([bq[nt * 16 + 4 * g:nt * 16 + 4 * g + 4] for g in G]).astype(np.float64)
            for kc in range(KC):
                acc = _k32(_wfrag(wqf, nt, kc), xq[kc], acc)
            for l in range(64):
                qkv[L15[l], nt * 16 + 4 * G[l]:nt * 16 + 4 * G[l] + 4] = acc[l]
        else:                                                        # operands swapped: D[token 4 g + r][feature l15]
            acc = np.stack([np.full(4, bq[nt * 16 + l15]) for l15 in L15]).astype(np.float64)
            for kc in range(KC):
                acc = _k32(xq[kc], _wfrag(wqf, nt, kc), acc)
            for l in range(64):
                qkv[4 * G[l]:4 * G[l] + 4, nt * 16 + L15[l]] = acc[l]
    return out, qkv


def test_f32_lanes_of_one_workgroup_reproduce_the_block_exactly():
    from lwdetr_amd import kernels as K
    gen = torch.Generator().manual_seed(5)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    x, att = ri(-3, 3, 16, C), ri(-2, 2, 16, C)
    wp, bp = ri(-2, 2, C, C), ri(-3, 3, C)
    w1, b1, w2, b2 = ri(-1, 1, HID, C), ri(-3, 3, HID), ri(-1, 1, C, HID), ri(-3, 3, C)
    ln2_w, ln2_b = ri(1, 2, C), ri(-1, 1, C)                         # integer affine: the fold stays exact
    wqkv, qb, vb = ri(-1, 1, 3 * C, C), ri(-3, 3, C), ri(-3, 3, C)
    ln1_w, ln1_b = ri(1, 2, C), ri(-1, 1, C)
    w1f, b1f, w2c = K.pack_mlp_weights(w1, b1, w2, ln2_w, ln2_b, torch.float32, proj=True)
    wq, bq = K.pack_qkv_weights(wqkv, qb, vb, ln1_w, ln1_b, torch.float32)
    w1F, wpF, wqF = K.pack_frag16(w1f), K.pack_frag16(wp), K.pack_frag16(wq)
    assert w1f.dtype == w2c.dtype == wq.dtype == torch.float32
    assert tuple(w1F.shape) == (HID // 16, KC, 16, 32) and tuple(wqF.shape) == (3 * C // 16, KC, 16, 32) and tuple(w2c.shape) == (HID // 32, C, 32)
    assert w1F[0, 0].numel() * w1F.element_size() == 2048            # an f32 fragment is one contiguous 2 KB
    d = lambda t: t.double().numpy()
    # the plain matrix formulation (no LayerNorm statistics, no activation, LayerScale 1)
    x1 = d(x) + d(att) @ d(wp).T + d(bp)
    hid = (x1 * d(ln2_w) + d(ln2_b)) @ d(w1).T + d(b1)
    ref_out = x1 + hid @ d(w2).T + d(b2)
    ref_qkv = (ref_out * d(ln1_w) + d(ln1_b)) @ d(wqkv).T + np.concatenate([d(qb), np.zeros(C), d(vb)])
    assert np.abs(ref_qkv).max() < 2.0 ** 52                         # every intermediate is an exactly representable integer
    args = (d(x), d(att), d(wpF), d(bp), d(w1F), d(b1f), d(w2c), d(b2), d(wqF), d(bq))
    out, qkv = _emulate_block(*args)
    assert np.array_equal(out, ref_out)
    assert np.array_equal(qkv, ref_qkv)
    # control: rows read back in natural k order (8 g + s) against the k-slot-permuted weights are a different product
    bad_out, bad_qkv = _emulate_block(*args, k_of=lambda g, h, e: 8 * g + 4 * h + e)
    assert not np.array_equal(bad_out, ref_out) and not np.array_equal(bad_qkv, ref_qkv)


# ---------------------------------------------------------------------------------------------------------------- (2) the Python predicates
F32 = torch.float32
BASE = dict(x=0x10000, ldx=192, att=0x20000, ldatt=192, w1=0x30000, b1=0x40000, w2=0x50000, b2=0x60000, gamma2=0x70000, wp=0x80000, bp=0x90000,
            gamma1=0xA0000, out2=0xB0000, ld2=384, wqkv=0xC0000, bqkv=0xD0000, q=0xE0000, k=0xF0000, vt=0x100000, heads=12, hd=16, Tp=400)
# one per refusal of lwdetr_vit_block_few with dtype 0: (M, C, changed arguments)
F32_REFUSED = {
    "C = 384": (1600, 384, {}),
    "M = 12800": (12800, 192, {}),
    "negative M": (-4, 192, {}),
    "ldx % 4": (1600, 192, dict(ldx=194)),
    "ld2 % 4": (1600, 192, dict(ld2=386)),
    "ldatt % 4": (1600, 192, dict(ldatt=198)),
    "x at an 8-byte offset": (1600, 192, dict(x=0x10008)),
    "att at an 8-byte offset": (1600, 192, dict(att=0x20008)),
    "out2 at an 8-byte offset": (1600, 192, dict(out2=0xB0008)),
    "q at an 8-byte offset": (1600, 192, dict(q=0xE0008)),
    "k at an 8-byte offset": (1600, 192, dict(k=0xF0008)),
    "vt at an 8-byte offset": (1600, 192, dict(vt=0x100008)),
    "w1 at an 8-byte offset": (1600, 192, dict(w1=0x30008)),
    "wp at an 8-byte offset": (1600, 192, dict(wp=0x80008)),
    "wqkv at an 8-byte offset": (1600, 192, dict(wqkv=0xC0008)),
    "w2 at an 8-byte offset": (1600, 192, dict(w2=0x50008)),
    "b1 at an 8-byte offset": (1600, 192, dict(b1=0x40008)),
    "b2 at an 8-byte offset": (1600, 192, dict(b2=0x60008)),
    "bp at an 8-byte offset": (1600, 192, dict(bp=0x90008)),
    "gamma1 at a 4-byte offset": (1600, 192, dict(gamma1=0xA0004)),
    "gamma2 at an 8-byte offset": (1600, 192, dict(gamma2=0x70008)),
    "bqkv at an 8-byte offset": (1600, 192, dict(bqkv=0xD0008)),
    "no attention output": (1600, 192, dict(att=None)),
    "no projection weight": (1600, 192, dict(wp=None)),
    "QKV without its bias": (1600, 192, dict(bqkv=None)),
    "QKV without a destination": (1600, 192, dict(vt=None)),
    "hd % 4": (1600, 192, dict(heads=32, hd=6)),
    "heads * hd != C": (1600, 192, dict(heads=6, hd=16)),
    "Tp % 4": (1600, 192, dict(Tp=402)),
    "M % 4 with QKV": (1602, 192, {}),
}


def test_vit_block_few_entry_takes_accepts_the_base_arguments():
    from lwdetr_amd import kernels as K
    for dt in (torch.float32, torch.float16, torch.bfloat16):
        assert K.vit_block_few_entry_takes(dt, 1600, 192, **BASE)
    assert not K.vit_block_few_entry_takes(torch.float64, 1600, 192, **BASE)
    assert K.vit_block_few_entry_takes(F32, 12796, 192, **BASE)
    # without the chained QKV and the tap copy: nothing of theirs is looked at, M need not be a multiple of 4
    bare = {**BASE, **dict(out2=None, ld2=0, wqkv=None, bqkv=None, q=None, k=None, vt=None, heads=0, hd=0, Tp=0)}
    assert K.vit_block_few_entry_takes(F32, 1602, 192, **bare)


@pytest.mark.parametrize("what", list(F32_REFUSED))
def test_vit_block_few_entry_takes_f32_mirrors_each_refusal(what):
    from lwdetr_amd import kernels as K
    m, c, kw = F32_REFUSED[what]
    assert not K.vit_block_few_entry_takes(F32, m, c, **{**BASE, **kw}), what


def test_vit_block_few_entry_takes_alignment_rules_differ_by_dtype():
    """f32: strides % 4 and 16-byte aligned operands; 16-bit: strides % 8, no pointer rule (the 16-bit kernel's widest access is 16 bytes of 8 values
    at multiples of 8 elements of rows the allocator aligns)."""
    from lwdetr_amd import kernels as K
    F16 = torch.float16
    for kw in (dict(ldx=196), dict(ldatt=196), dict(ld2=388)):
        assert K.vit_block_few_entry_takes(F32, 1600, 192, **{**BASE, **kw}) and not K.vit_block_few_entry_takes(F16, 1600, 192, **{**BASE, **kw}), kw
    assert K.vit_block_few_entry_takes(F16, 1600, 192, **{**BASE, "x": 0x10008}) and not K.vit_block_few_entry_takes(F32, 1600, 192, **{**BASE, "x": 0x10008})


def test_vit_block_few_supported_takes_f32_only_behind_its_switch(monkeypatch):
    from lwdetr_amd import kernels as K
    F16 = torch.float16
    for v in ("LWDETR_VIT_BLOCK_FEW_F32", "LWDETR_VIT_BLOCK_FEW", "LWDETR_MLP_FUSED"):
        monkeypatch.delenv(v, raising=False)
    assert 0 < K.VIT_BLOCK_FEW_F32_MAX_ROWS <= 12800
    lim = K.VIT_BLOCK_FEW_F32_MAX_ROWS
    assert not K.vit_block_few_supported(192, F32, 1600)             # the default: off
    assert K.vit_block_few_supported(192, F16, 1600)
    # mlp_fused_supported without the switch: what it returned before the f32 form existed
    present = {64: False, 1600: False, 12799: False, 12800: True, 51200: True}
    for rows, val in present.items():
        assert K.mlp_fused_supported(192, F32, rows) is val, rows
        assert K.mlp_fused_supported(192, F16, rows) is True
        assert K.mlp_fused_supported(384, F32, rows) is False
    assert K.mlp_fused_supported(192, F32) is True and K.mlp_fused_supported(384, F32) is False
    monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW_F32", "0")
    assert not K.vit_block_few_supported(192, F32, 1600) and not K.mlp_fused_supported(192, F32, 1600)
    monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW_F32", "1")
    assert K.vit_block_few_supported(192, F32, 1600) and K.vit_block_few_supported(192, F32, 64) and K.vit_block_few_supported(192, F32, lim - 1)
    assert not K.vit_block_few_supported(384, F32, 1600)
    assert not K.vit_block_few_supported(192, F32, lim) and not K.vit_block_few_supported(192, F32, 51200)
    assert not K.vit_block_few_supported(192, F32, None)
    assert not K.vit_block_few_supported(192, torch.float64, 1600)
    assert K.vit_block_few_supported(192, F16, 1600) and not K.vit_block_few_supported(192, F16, 12800)
    # the plan follows: fused below MLP_FUSED_MIN_ROWS exactly where the few-token kernel is taken
    for rows in (64, 1600, 12799, 12800, 51200):
        assert K.mlp_fused_supported(192, F32, rows) is (rows >= K.MLP_FUSED_MIN_ROWS or rows < lim), rows
        assert K.mlp_fused_supported(384, F32, rows) is False
    monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW", "0")                  # the A/B switch of the 16-bit form keeps every dtype off the kernel
    assert not K.vit_block_few_supported(192, F32, 1600) and not K.vit_block_few_supported(192, F16, 1600)
    assert not K.mlp_fused_supported(192, F32, 1600)


# ---------------------------------------------------------------------------------------------------------------- (3) registers of the build
def test_f32_vit_block_few_kernels_use_no_scratch():
    """Every mlp_small_kernel<float, ...> of the built library (QKV true / false, TT = 1, FRAG): no scratch, no spilled registers, within the 256 registers
    a wave of a 512-thread workgroup has. The 16-bit instantiations are found by the same walk and printed with their counts."""
    from lwdetr_amd import _native
    assert _native.is_built(), f"{_native.LIB_PATH} is not built"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    table = [r for r in kernel_regs.kernel_table(_native.LIB_PATH) if "mlp_small_kernelI" in r["symbol"]]
    f32 = [r for r in table if "mlp_small_kernelIf" in r["symbol"]]  # Itanium mangling: If = <float
    forms = sorted(r["symbol"].split("mlp_small_kernelIf")[1][:15] for r in f32)
    assert forms == ["Lb0ELi1ELb1EEEv", "Lb1ELi1ELb1EEEv"], [r["symbol"] for r in f32]       # (QKV, TT = 1, FRAG = true)
    for r in f32:
        print("f32   ", r["symbol"], {k: r[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0, r
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["vgpr_count"] is not None and r["vgpr_count"] + (r["agpr_count"] or 0) <= 256, r
    b16 = [r for r in table if "mlp_small_kernelID" in r["symbol"]]  # DF16_ = _Float16, DF16b = __bf16
    for r in b16:
        print("16-bit", r["symbol"], {k: r[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size")})
    assert len(b16) == 16, len(b16)                                  # 2 dtypes x QKV x TT x FRAG
    assert all(r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 for r in b16)
