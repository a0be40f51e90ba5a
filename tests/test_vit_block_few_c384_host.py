"""CPU: the host side of the C = 384 form of lwdetr_vit_block_few (vit_block_few384_kernel, lw-detr_amd/csrc/vit_block_few384.hip).

(1) A lane-level numpy emulation of the data flow of one 16-token workgroup on small integers (every sum is exact): wave w's three projection tiles ->
    x1 rows in LDS -> every wave's B fragments in k-slot order -> wave w's twelve hidden tiles of fc1 on pack_frag16(pack_mlp_weights(proj=True)) -> the
    hidden rows in LDS -> the B fragment of a hidden chunk as two 4-value reads (hidden 4 g .., 16 + 4 g ..) -> fc2 on the chunk-major w2c for wave w's
    three channel tiles over all 48 chunks, four chunks per register batch -> the new rows in LDS -> QKV on pack_frag16(pack_qkv_weights), feature tiles
    w, w + 8, .., V^T with the operands swapped. It equals the plain matrix formulation exactly on the existing packers' output; two controls with a wrong
    k-slot order (rows read back in natural order; the hidden fragment read as one run of 8) do not. (LayerNorm and GELU act per element / per row
    between the products and are left out: identity affine, no activation.)
(2) kernels.vit_block_few_supported / mlp_fused_supported / vit_block_few_entry_takes at C = 384 and the plan switch LWDETR_VIT_BLOCK_FEW_C384.
(3) tools/kernel_regs.py on the built library: no vit_block_few384_kernel spills or uses scratch (metadata only, no GPU)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C, KC, NT, HID, NW = 384, 12, 24, 1536, 8
NCH, NTW, HTW, CB = HID // 32, NT // NW, HID // 16 // NW, 4
L15 = np.arange(64) & 15
G = np.arange(64) >> 4


# ---------------------------------------------------------------------------------------------------------------- (1) lane-level emulation
def _k32(a, b, acc):
    """One 16x16x32 MFMA: a, b (64 lanes, 8 values) - lane (l15, g) holds k = 8 g .. 8 g + 7 of row / column l15 -, acc (64, 4): D[4 g + r][l15]."""
    A, B = np.zeros((16, 32)), np.zeros((32, 16))
    for l in range(64):
        A[L15[l], 8 * G[l]:8 * G[l] + 8] = a[l]
        B[8 * G[l]:8 * G[l] + 8, L15[l]] = b[l]
    D = A @ B
    return acc + np.stack([D[4 * G[l]:4 * G[l] + 4, L15[l]] for l in range(64)])


def _frag(flat, idx):
    """Fragment `idx` of a fragment-major array as the kernel loads it: lane (l15, g) reads 8 values at idx * 512 + l15 * 32 + g * 8."""
    return np.stack([flat[idx * 512 + l15 * 32 + g * 8:idx * 512 + l15 * 32 + g * 8 + 8] for l15, g in zip(L15, G)])


def _rows_as_bfrag(rows, kc, k_of):
    """Rows [16][C] in LDS -> the B fragment of k-chunk kc: lane (token l15, g), slot h * 4 + e <- channel 32 kc + k_of(g, h, e)."""
    return np.stack([[rows[l15, 32 * kc + k_of(g, h, e)] for h in range(2) for e in range(4)] for l15, g in zip(L15, G)])


KSLOT = lambda g, h, e: 16 * h + 4 * g + e                               # what the kernel reads: two 4-value runs
NATURAL = lambda g, h, e: 8 * g + 4 * h + e                              # the wrong order of the controls


def _emulate_block(x, att, wpf, bp, w1f, b1, w2c, b2, wqf, bq, x_of=KSLOT, h_of=KSLOT):
    """One workgroup of vit_block_few384_kernel without LayerNorm / GELU / LayerScale: (new rows [16][C], q | k | v as [token][feature])."""
    wpf, w1f, w2c, wqf = (a.reshape(-1) for a in (wpf, w1f, w2c, wqf))
    x1s, hs = np.zeros((16, C)), np.zeros((16, HID))
    af = [np.stack([att[l15, 32 * kc + 8 * g:32 * kc + 8 * g + 8] for l15, g in zip(L15, G)]) for kc in range(KC)]
    for wave in range(NW):                                               # projection: channel tiles 3 w .. 3 w + 2
        for i in range(NTW):
            n = wave * NTW + i
            acc = np.zeros((64, 4))
            for kc in range(KC):
                acc = _k32(_frag(wpf, n * KC + kc), af[kc], acc)
            for l in range(64):                                          # accumulator lane (token l15, g): channels 4 g .. 4 g + 3 of the tile
                c0 = n * 16 + 4 * G[l]
                x1s[L15[l], c0:c0 + 4] = x[L15[l], c0:c0 + 4] + acc[l] + bp[c0:c0 + 4]
    xf = [_rows_as_bfrag(x1s, kc, x_of) for kc in range(KC)]
    for wave in range(NW):                                               # fc1: hidden tiles 12 w .. 12 w + 11 -> hs
        for it in range(HTW):
            ht = wave * HTW + it
            acc = np.stack([b1[ht * 16 + 4 * g:ht * 16 + 4 * g + 4] for g in G]).astype(np.float64)
            for kc in range(KC):
                acc = _k32(_frag(w1f, ht * KC + kc), xf[kc], acc)
            for l in range(64):
                hs[L15[l], ht * 16 + 4 * G[l]:ht * 16 + 4 * G[l] + 4] = acc[l]
    for wave in range(NW):                                               # fc2: channel tiles 3 w .. over all chunks, CB chunks per batch
        n0 = wave * NTW
        acc2 = [np.zeros((64, 4)) for _ in range(NTW)]
        for hc0 in range(0, NCH, CB):
            batch = [_frag(w2c, (hc0 + j) * NT + n0 + i) for j in range(CB) for i in range(NTW)]
            for j in range(CB):
                hf = _rows_as_bfrag(hs, hc0 + j, h_of)
                for i in range(NTW):
                    acc2[i] = _k32(batch[j * NTW + i], hf, acc2[i])
        for i in range(NTW):
            for l in range(64):
                c0 = (n0 + i) * 16 + 4 * G[l]
                x1s[L15[l], c0:c0 + 4] += acc2[i][l] + b2[c0:c0 + 4]
    out = x1s.copy()
    xq = [_rows_as_bfrag(x1s, kc, x_of) for kc in range(KC)]
    qkv = np.zeros((16, 3 * C))
    for wave in range(NW):
        for it in range(3 * C // 16 // NW):
            nt = wave + it * NW
            if nt // NT < 2:                                             # D[feature 4 g + r][token l15]
                acc = np.stack([bq[nt * 16 + 4 * g:nt * 16 + 4 * g + 4] for g in G]).astype(np.float64)
                for kc in range(KC):
                    acc = _k32(_frag(wqf, nt * KC + kc), xq[kc], acc)
                for l in range(64):
                    qkv[L15[l], nt * 16 + 4 * G[l]:nt * 16 + 4 * G[l] + 4] = acc[l]
            else:                                                        # operands swapped: D[token 4 g + r][feature l15]
                acc = np.stack([np.full(4, bq[nt * 16 + l15]) for l15 in L15]).astype(np.float64)
                for kc in range(KC):
                    acc = _k32(xq[kc], _frag(wqf, nt * KC + kc), acc)
                for l in range(64):
                    qkv[4 * G[l]:4 * G[l] + 4, nt * 16 + L15[l]] = acc[l]
    return out, qkv


def test_c384_lanes_of_one_workgroup_reproduce_the_block_exactly():
    from lwdetr_amd import kernels as K
    gen = torch.Generator().manual_seed(11)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    x, att = ri(-3, 3, 16, C), ri(-2, 2, 16, C)
    wp, bp = ri(-2, 2, C, C), ri(-3, 3, C)
    w1, b1, w2, b2 = ri(-1, 1, HID, C), ri(-3, 3, HID), ri(-1, 1, C, HID), ri(-3, 3, C)
    ln2_w, ln2_b = ri(1, 2, C), ri(-1, 1, C)                         # integer affine: the fold stays exact
    wqkv, qb, vb = ri(-1, 1, 3 * C, C), ri(-3, 3, C), ri(-3, 3, C)
    ln1_w, ln1_b = ri(1, 2, C), ri(-1, 1, C)
    w1f, b1f, w2c = K.pack_mlp_weights(w1, b1, w2, ln2_w, ln2_b, torch.float32, proj=True)     # small integers: exact in f16 / bf16 as well
    wq, bq = K.pack_qkv_weights(wqkv, qb, vb, ln1_w, ln1_b, torch.float32)
    w1F, wpF, wqF = K.pack_frag16(w1f), K.pack_frag16(wp), K.pack_frag16(wq)
    assert tuple(w1F.shape) == (HID // 16, KC, 16, 32) and tuple(wpF.shape) == (NT, KC, 16, 32) and tuple(wqF.shape) == (3 * NT, KC, 16, 32)
    assert tuple(w2c.shape) == (NCH, C, 32)
    assert torch.equal(w1f.half().float(), w1f) and torch.equal(w2c.bfloat16().float(), w2c)
    d = lambda t: t.double().numpy()
    x1 = d(x) + d(att) @ d(wp).T + d(bp)
    hid = (x1 * d(ln2_w) + d(ln2_b)) @ d(w1).T + d(b1)
    ref_out = x1 + hid @ d(w2).T + d(b2)
    ref_qkv = (ref_out * d(ln1_w) + d(ln1_b)) @ d(wqkv).T + np.concatenate([d(qb), np.zeros(C), d(vb)])
    assert np.abs(ref_qkv).max() < 2.0 ** 52                         # every intermediate is an exactly representable integer
    args = (d(x), d(att), d(wpF), d(bp), d(w1F), d(b1f), d(w2c), d(b2), d(wqF), d(bq))
    out, qkv = _emulate_block(*args)
    assert np.array_equal(out, ref_out)
    assert np.array_equal(qkv, ref_qkv)
    # control 1: the x1 rows read back in natural k order against the k-slot-permuted fc1 / QKV weights
    bad_out, bad_qkv = _emulate_block(*args, x_of=NATURAL)
    assert not np.array_equal(bad_out, ref_out) and not np.array_equal(bad_qkv, ref_qkv)
    # control 2: the hidden fragment read as one run of 8 per lane group against the k-slot order baked into w2c
    bad_out, _ = _emulate_block(*args, h_of=NATURAL)
    assert not np.array_equal(bad_out, ref_out)


# ---------------------------------------------------------------------------------------------------------------- (2) the Python predicates
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
BASE = dict(x=0x10000, ldx=384, att=0x20000, ldatt=384, w1=0x30000, b1=0x40000, w2=0x50000, b2=0x60000, gamma2=0x70000, wp=0x80000, bp=0x90000,
            gamma1=0xA0000, out2=0xB0000, ld2=768, wqkv=0xC0000, bqkv=0xD0000, q=0xE0000, k=0xF0000, vt=0x100000, heads=12, hd=32, Tp=400)
# one per 16-bit refusal of lwdetr_vit_block_few at C = 384: (M, C, changed arguments)
REFUSED = {
    "C = 768": (1600, 768, dict(heads=24)),
    "M = 12800": (12800, 384, {}),
    "negative M": (-4, 384, {}),
    "ldx % 8": (1600, 384, dict(ldx=388)),
    "ld2 % 8": (1600, 384, dict(ld2=772)),
    "ldatt % 8": (1600, 384, dict(ldatt=388)),
    "no attention output": (1600, 384, dict(att=None)),
    "no projection weight": (1600, 384, dict(wp=None)),
    "QKV without its bias": (1600, 384, dict(bqkv=None)),
    "QKV without a destination": (1600, 384, dict(vt=None)),
    "hd % 4": (1600, 384, dict(heads=64, hd=6)),
    "heads * hd != C": (1600, 384, dict(heads=6, hd=32)),
    "Tp % 4": (1600, 384, dict(Tp=402)),
    "M % 4 with QKV": (1602, 384, {}),
}


def _clear(monkeypatch):
    for v in ("LWDETR_VIT_BLOCK_FEW_C384", "LWDETR_VIT_BLOCK_FEW_F32", "LWDETR_VIT_BLOCK_FEW", "LWDETR_MLP_FUSED"):
        monkeypatch.delenv(v, raising=False)


def test_entry_takes_16_bit_c384_and_never_float32():
    from lwdetr_amd import kernels as K
    for dt in (F16, BF16):
        assert K.vit_block_few_entry_takes(dt, 1600, 384, **BASE)
        assert K.vit_block_few_entry_takes(dt, 12796, 384, **BASE)
    assert not K.vit_block_few_entry_takes(F32, 1600, 384, **BASE)
    bare = {**BASE, **dict(out2=None, ld2=0, wqkv=None, bqkv=None, q=None, k=None, vt=None, heads=0, hd=0, Tp=0)}
    assert K.vit_block_few_entry_takes(F16, 1602, 384, **bare) and not K.vit_block_few_entry_takes(F32, 1602, 384, **bare)
    assert K.vit_block_few_entry_takes(F16, 1600, 384, **{**BASE, "x": 0x10008})       # 16-bit: no pointer rule, as at C = 192


@pytest.mark.parametrize("what", list(REFUSED))
def test_entry_takes_mirrors_each_16_bit_refusal_at_c384(what):
    from lwdetr_amd import kernels as K
    m, c, kw = REFUSED[what]
    for dt in (F16, BF16):
        assert not K.vit_block_few_entry_takes(dt, m, c, **{**BASE, **kw}), what


def test_c384_is_off_by_default_and_on_only_behind_its_switch(monkeypatch):
    from lwdetr_amd import kernels as K
    _clear(monkeypatch)
    lim = K.VIT_BLOCK_FEW_C384_MAX_ROWS
    assert 0 < lim <= K.VIT_BLOCK_FEW_MAX_ROWS
    rows_all = (64, 1600, 12799, 12800, 51200)
    today = {64: False, 1600: False, 12799: False, 12800: True, 51200: True}         # mlp_fused_supported(384, 16-bit, rows) before this kernel existed
    c192 = {dt: [(K.vit_block_few_supported(192, dt, r), K.mlp_fused_supported(192, dt, r)) for r in rows_all] for dt in (F16, BF16, F32)}
    for dt in (F16, BF16):
        for rows in rows_all:
            assert not K.vit_block_few_supported(384, dt, rows)
            assert K.mlp_fused_supported(384, dt, rows) is today[rows], (dt, rows)
        assert K.mlp_fused_supported(384, dt) is True
    monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW_C384", "0")
    assert not K.vit_block_few_supported(384, F16, 64) and K.mlp_fused_supported(384, F16, 1600) is False
    monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW_C384", "1")
    for dt in (F16, BF16):
        assert K.vit_block_few_supported(384, dt, 64) and K.vit_block_few_supported(384, dt, lim - 1)
        assert not K.vit_block_few_supported(384, dt, lim) and not K.vit_block_few_supported(384, dt, 12800) and not K.vit_block_few_supported(384, dt, 51200)
        assert not K.vit_block_few_supported(384, dt, None)
        for rows in rows_all:                                            # the plan follows: fused exactly where the few-token kernel is taken
            assert K.mlp_fused_supported(384, dt, rows) is (rows >= K.MLP_FUSED_MIN_ROWS or rows < lim), (dt, rows)
    for rows in rows_all:                                                # never float32 at C = 384, under any switch
        assert not K.vit_block_few_supported(384, F32, rows) and K.mlp_fused_supported(384, F32, rows) is False
    monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW_F32", "1")
    assert not K.vit_block_few_supported(384, F32, 64) and K.mlp_fused_supported(384, F32, 64) is False
    monkeypatch.delenv("LWDETR_VIT_BLOCK_FEW_F32")
    # C = 192 answers are unchanged by the switch
    assert c192 == {dt: [(K.vit_block_few_supported(192, dt, r), K.mlp_fused_supported(192, dt, r)) for r in rows_all] for dt in (F16, BF16, F32)}
    assert not K.vit_block_few_supported(768, F16, 64)
    monkeypatch.setenv("LWDETR_VIT_BLOCK_FEW", "0")                      # the A/B switch of the C = 192 form wins
    assert not K.vit_block_few_supported(384, F16, 64) and not K.vit_block_few_supported(384, BF16, 64)
    assert K.mlp_fused_supported(384, F16, 64) is False and K.mlp_fused_supported(384, F16, 12800) is True


# ---------------------------------------------------------------------------------------------------------------- (3) registers of the build
def test_c384_vit_block_few_kernels_use_no_scratch():
    """Every vit_block_few384_kernel of the built library (f16 / bf16 x QKV): no scratch, no spilled registers, within the 256 registers a wave of a
    512-thread workgroup has."""
    from lwdetr_amd import _native
    assert _native.is_built(), f"{_native.LIB_PATH} is not built"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_regs
    finally:
        sys.path.pop(0)
    table = [r for r in kernel_regs.kernel_table(_native.LIB_PATH) if "vit_block_few384_kernelI" in r["symbol"]]
    forms = sorted(r["symbol"].split("vit_block_few384_kernelI")[1].split("EEEv")[0] for r in table)
    assert forms == ["DF16_Lb0", "DF16_Lb1", "DF16bLb0", "DF16bLb1"], [r["symbol"] for r in table]   # Itanium: DF16_ = _Float16, DF16b = __bf16; QKV
    for r in table:
        print(r["symbol"], {k: r[k] for k in ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "private_segment_fixed_size")})
        assert r["private_segment_fixed_size"] == 0, r
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
        assert r["vgpr_count"] is not None and r["vgpr_count"] + (r["agpr_count"] or 0) <= 256, r
