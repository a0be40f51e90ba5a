"""CPU: the case table of the plan-shape tests holds what it claims (tests/plan_shapes_cases.py), and the comparator of
tests/test_gpu_plan_shapes.py (b) - ours <= 1.5 x the reference's own 16-bit error, max and mean, per tensor and batch slot - BITES: wiring mistakes
of the kind those tests exist for are planted into the fp32 oracle (oracle/lwdetr_torch.py with one function replaced: the mistake's pure effect, no
16-bit noise on top) on the two images of case l384p (large, 384 x 320, padded, Tw = 30 -> Twp = 32, P3 + P5), and each must push a ratio past 1.5.

Planted, and the ratio it reaches (worst tensor; recorded by the test in its assertion message when it fails to bite):
  * one window's pad row used as a key (window 0 of image 0, every window block; the pad row modelled as a zero token: k = 0, v = v_bias)
  * the P5 level offset by one row (the sampling core reads level 1 from one memory row early)
  * notpad taken from the other image (the value rows are zeroed with the other image's padding mask)
  * valid ratios swapped between x and y
  * the position table in raster order instead of window-major
All five are visible to this comparator at fp16 on this case (none had to be listed as "not visible to this comparator")."""
import numpy as np
import pytest
import torch

import lwdetr_amd
import plan_shapes_cases as P
from plan_shapes_cases import CASES

PLANT_CASE = "l384p"


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_reaches_the_fused_plan_by_arithmetic(case):
    from lwdetr_amd import kernels as K
    from lwdetr_amd.configs import VIT_SIZES
    assert case.H % 64 == 0 and case.W % 64 == 0
    # ForwardPlan's formulas, restated (engine.py: Hp = H / 16, 4 x 4 windows of h x w tokens, every window padded to ceil4 rows)
    hp, wp = case.H // 16, case.W // 16
    h, w = hp // 4, wp // 4
    tw = h * w
    twp = (tw + 3) // 4 * 4
    assert (case.Tw, case.Twp, case.Tp, case.rows) == (tw, twp, 16 * twp, case.B * 16 * twp)
    geo = P.plan_geometry(case.size, case.H, case.W)
    assert (geo["Tw"], geo["Twp"], geo["Tp"]) == (tw, twp, 16 * twp)
    assert case.rows >= 12800 == K.VIT_BLOCK_MIN_ROWS == K.MLP_FUSED_MIN_ROWS and case.rows % 8 == 0
    assert case.B * geo["S"] >= 2048 == K.CHAIN_MIN_ROWS
    assert geo["S"] >= geo["nq"]
    cfg = lwdetr_amd.get_args(case.size)
    C = VIT_SIZES[cfg.encoder][0]
    if case.dtype == "float32":
        assert C == 192 and K.mlp_fused_supported(C, torch.float32, case.rows) and not K.vit_block_supported(C, torch.float32, C // 12, case.rows)
    else:
        assert K.vit_block_supported(C, P.dtype_of(case), C // 12, case.rows) and K.mlp_fused_supported(C, P.dtype_of(case), case.rows)
        assert K.enc_chain_supported(cfg.hidden_dim, P.dtype_of(case), ncls=91, nl=cfg.dec_layers, rows=case.B * geo["S"])
    if case.valid is not None:
        assert len(case.valid) == 2 and all(0 < a <= case.H and 0 < b <= case.W for a, b in case.valid)
        assert any((a, b) != (case.H, case.W) for a, b in case.valid) and max(a for a, _ in case.valid) == case.H and max(b for _, b in case.valid) == case.W
        x, m = P.case_images(case)
        assert m.any() and (x.permute(0, 2, 3, 1)[m] == 0).all() and not m[0, :case.valid[0][0], :case.valid[0][1]].any()


def test_table_covers_the_shape_classes():
    assert len({c.id for c in CASES}) == len(CASES) and len({c.seed for c in CASES}) == len(CASES)
    assert sum(c.Twp != c.Tw for c in CASES) >= 4
    assert sum(c.valid is not None for c in CASES) >= 3
    assert sum(c.B % 2 == 1 for c in CASES) >= 2
    assert sum(c.Tp % 128 != 0 for c in CASES) >= 1
    assert sum(c.H != c.W for c in CASES) >= 3
    assert {c.dtype for c in CASES} == {"float16", "bfloat16", "float32"}
    for name in P.SENTINEL_CASES + P.PADSTATE_CASES + P.ARENA_CASES:
        assert name in P.BY_ID
    assert all(P.BY_ID[n].valid is not None for n in P.PADSTATE_CASES)


def test_tile_alternates_the_two_images():
    t = torch.arange(2)[:, None].expand(2, 3)
    for B in (7, 26):
        assert P.tile(t, B)[:, 0].tolist() == [k % 2 for k in range(B)]
    assert P.tile(None, 5) is None


@pytest.mark.parametrize("hw", sorted({(c.H, c.W) for c in CASES}))
def test_winmajor_rows_reproduce_the_order_of_the_position_table(hw):
    """The row index the GPU test reads `x` / `taps_cat` through, against engine.abs_pos_winmajor on a random position table: the indexed rows are the
    oracle's windowed token order, every other row of the table is a zero pad row."""
    from lwdetr_amd.engine import abs_pos_winmajor
    from oracle import lwdetr_torch as O
    hp, wp = hw[0] // 16, hw[1] // 16
    h, w = hp // 4, wp // 4
    twp = (h * w + 3) // 4 * 4
    c = 8
    pos = torch.randn(1, 1 + 14 * 14, c, generator=torch.Generator().manual_seed(hp * 100 + wp))
    table = abs_pos_winmajor(pos, hp, wp, twp)
    assert table.shape == (16 * twp, c)
    ras = O.abs_pos(pos, hp, wp)                                                                        # (1, hp, wp, c) raster
    want = ras.reshape(1, 4, h, 4, w, c).permute(0, 1, 3, 2, 4, 5).reshape(16 * h * w, c)              # oracle/lwdetr_torch.py:vit windowing
    rows = P.winmajor_rows(hp, wp, twp)
    assert len(rows) == 16 * h * w == len(set(rows.tolist()))
    assert torch.equal(table[rows], want)
    rest = np.setdiff1d(np.arange(16 * twp), rows)
    assert len(rest) == 16 * (twp - h * w) and (table[rest] == 0).all()


def test_ratio_arithmetic_on_a_made_up_tensor():
    t32 = {"a": np.zeros((2, 4), np.float32)}
    t16 = {"a": np.array([[0.1, 0, 0, 0], [0.2, 0.2, 0.2, 0.2]], np.float32)}
    y = P.yardstick(t32, t16)
    assert np.allclose(y["a"]["max"], [0.1, 0.2]) and np.allclose(y["a"]["mean"], [0.025, 0.2])
    ours = {"a": np.array([[0.05, 0, 0, 0], [0.1, 0.1, 0.1, 0.1], [0.3, 0, 0, 0]], np.float32)}      # slot 2 holds image 0 again
    r = P.ratios(ours, t32, y)["a"]
    assert np.isclose(r["max"], 3.0) and r["slot_max"] == 2 and np.isclose(r["mean"], 3.0) and r["slot_mean"] == 2
    assert P.worst({"a": r})[0] == pytest.approx(3.0)


# ------------------------------------------------------------------------------------------------- planted mistakes
@pytest.fixture(scope="module")
def plant():
    """fp32 oracle, fp16 oracle (the yardstick) and a runner for a patched fp32 oracle on the two images of PLANT_CASE."""
    from helpers import oracle_lowp
    from lwdetr_amd.synth import synth_state_dict
    from oracle import lwdetr_torch as O
    case = P.BY_ID[PLANT_CASE]
    geo = P.plan_geometry(case.size, case.H, case.W)
    x, mask = P.case_images(case)
    c32, c16 = {}, {}
    ref32 = oracle_lowp(case.size, 0, 0, 0, torch.float32, None, images=x, mask=mask, collect=c32)
    ref16 = oracle_lowp(case.size, 0, 0, 0, P.dtype_of(case), ref32["topk_idx"], images=x, mask=mask, collect=c16)
    t32, t16 = P.oracle_tensors(ref32, c32, geo), P.oracle_tensors(ref16, c16, geo)
    yard = P.yardstick(t32, t16)
    cfg = lwdetr_amd.get_args(case.size)
    model, _, _ = lwdetr_amd.build_model(cfg)
    sd = synth_state_dict(model.state_dict(), seed=0)
    forced = torch.from_numpy(ref32["topk_idx"])

    def run(monkeypatch, **patches):
        for name, fn in patches.items():
            monkeypatch.setattr(O, name, fn)
        col = {}
        with torch.no_grad():
            out = O.forward(sd, cfg, x, mask, forced_topk=forced, collect=col)
        f = lambda t: t.float().numpy()
        ref = {"pred_logits": f(out["pred_logits"]), "pred_boxes": f(out["pred_boxes"]), "enc_logits": f(out["enc_outputs"]["pred_logits"]),
               "enc_boxes": f(out["enc_outputs"]["pred_boxes"]), "aux_logits": np.stack([f(a["pred_logits"]) for a in out["aux_outputs"]], 1),
               "aux_boxes": np.stack([f(a["pred_boxes"]) for a in out["aux_outputs"]], 1)}
        return P.ratios(P.oracle_tensors(ref, {k: f(v) for k, v in col.items()}, geo), t32, yard)

    return dict(case=case, geo=geo, mask=mask, run=run, O=O, t32=t32, t16=t16, yard=yard)


def test_unplanted_oracle_and_the_yardstick_itself(plant, monkeypatch):
    """Nothing planted: every ratio is 0; the 16-bit oracle against its own yardstick: every ratio is 1 - the comparator's two fixed points."""
    r = plant["run"](monkeypatch)
    assert P.worst(r)[0] == 0.0
    r = P.ratios(plant["t16"], plant["t32"], plant["yard"])
    assert all(abs(v[c] - 1.0) < 1e-9 for v in r.values() for c in ("max", "mean")), r


def _bites(r, front=None):
    w = P.worst(r)
    assert w[0] > P.RATIO, f"planted mistake not visible to this comparator: worst ratio {w}"
    if front is not None:       # the stage where the mistake is made shows it, not only the outputs behind it
        assert max(r[front]["max"], r[front]["mean"]) > P.RATIO, (front, r[front])
    return w


def test_planted_pad_row_used_as_a_key(plant, monkeypatch):
    O, geo = plant["O"], plant["geo"]
    import torch.nn.functional as F

    def vit_attention(sd, pre, x, heads):
        n_seq, n_tok, c = x.shape
        hd = c // heads
        bias = torch.cat([sd[pre + ".q_bias"], torch.zeros_like(sd[pre + ".v_bias"]), sd[pre + ".v_bias"]])
        qkv = F.linear(x, sd[pre + ".qkv.weight"], bias).reshape(n_seq, n_tok, 3, heads, hd).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        s = (q * hd ** -0.5) @ k.transpose(-2, -1)
        out = s.softmax(-1) @ v
        if n_tok == geo["Tw"]:                   # a window block: window 0 of image 0 also sees one pad row (a zero token: k = 0, v = v_bias)
            s0 = torch.cat([s[0], torch.zeros_like(s[0][..., :1])], -1).softmax(-1)
            v0 = torch.cat([v[0], sd[pre + ".v_bias"].reshape(heads, 1, hd)], 1)
            out = torch.cat([(s0 @ v0)[None], out[1:]], 0)
        return O._lin(sd, pre + ".proj", out.transpose(1, 2).reshape(n_seq, n_tok, c))

    r = plant["run"](monkeypatch, vit_attention=vit_attention)
    _bites(r, front=f"vit.block{geo['taps'][0]}")


def test_planted_p5_level_offset_by_one_row(plant, monkeypatch):
    O, geo = plant["O"], plant["geo"]
    import torch.nn.functional as F
    assert len(geo["level_hw"]) == 2

    def msda_core(value, shapes, loc, aw):
        b, _, m, d = value.shape
        q = loc.shape[1]
        out = value.new_zeros(b, q, m, d)
        cur = 0
        for lvl, (hl, wl) in enumerate(shapes):
            c0 = cur - 1 if lvl == 1 else cur                                          # the planted mistake
            v = value[:, c0:c0 + hl * wl].permute(0, 2, 3, 1).reshape(b * m, d, hl, wl)
            grid = (2 * loc[:, :, :, lvl] - 1).transpose(1, 2).flatten(0, 1)
            samp = F.grid_sample(v, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
            w = aw[:, :, :, lvl].transpose(1, 2).reshape(b * m, 1, q, -1)
            out += (samp * w).sum(-1).view(b, m, d, q).permute(0, 3, 1, 2)
            cur += hl * wl
        return out.reshape(b, q, m * d)

    r = plant["run"](monkeypatch, msda_core=msda_core)
    assert max(r["memory"]["max"], r["enc.class_max"]["max"]) == 0.0                   # the stages in front of the decoder do not see it
    _bites(r, front="hs0")


def test_planted_notpad_from_the_other_image(plant, monkeypatch):
    O = plant["O"]
    real = O.msda
    r = plant["run"](monkeypatch, msda=lambda sd, pre, query, ref, memory, mask_flat, shapes, nh, npt:
                     real(sd, pre, query, ref, memory, mask_flat.flip(0), shapes, nh, npt))
    _bites(r, front="hs0")


def test_planted_valid_ratios_swapped(plant, monkeypatch):
    O, geo, mask = plant["O"], plant["geo"], plant["mask"]
    import torch.nn.functional as F
    masks = [F.interpolate(mask[None].float(), size=s).to(torch.bool)[0] for s in geo["level_hw"]]
    vr = torch.stack([torch.stack([(~m[:, 0, :]).sum(1).float() / m.shape[2], (~m[:, :, 0]).sum(1).float() / m.shape[1]], -1) for m in masks], 1)
    assert (vr[..., 0] != vr[..., 1]).any()                                            # (B, L, 2): some image has another ratio in x than in y
    fix = (vr.flip(-1) / vr).repeat(1, 1, 2)[:, None]                                  # ref * vr -> ref * swapped vr: (B, 1, L, 4)
    real_msda, real_sine = O.msda, O.sine_embed
    r = plant["run"](monkeypatch,
                     msda=lambda sd, pre, query, ref, *a: real_msda(sd, pre, query, ref * fix, *a),
                     sine_embed=lambda pos, dim: real_sine(pos * fix[:, :, 0], dim))
    _bites(r, front="hs0")


def test_planted_position_table_in_raster_order(plant, monkeypatch):
    O, geo = plant["O"], plant["geo"]
    real = O.abs_pos
    hp, wp = geo["Hp"], geo["Wp"]
    h, w = hp // 4, wp // 4
    # window-major index (no pad rows) of raster token (y, x): the mistaken plan adds raster-table row m to the token at window-major row m
    yy, xx = np.meshgrid(np.arange(hp), np.arange(wp), indexing="ij")
    m = (((yy // h) * 4 + xx // w) * (h * w) + (yy % h) * w + xx % w).reshape(-1)
    assert sorted(m.tolist()) == list(range(hp * wp)) and (m != np.arange(hp * wp)).any()

    def abs_pos(pos_embed, hp_, wp_):
        p = real(pos_embed, hp_, wp_)
        return p.reshape(hp * wp, -1)[torch.from_numpy(m)].reshape(p.shape)

    r = plant["run"](monkeypatch, abs_pos=abs_pos)
    _bites(r, front=f"vit.block{geo['taps'][0]}")
