"""Case table of the plan-shape tests (tests/test_plan_shapes_host.py, tests/test_gpu_plan_shapes.py): the batch shapes at which ForwardPlan takes its
fused 16-bit kernels (rows = B * Tp >= 12800: stem, VitBlockOp, fused MLP; B * S >= 2048: the encoder chain) AWAY from the one shape class every other
model-level test runs them at (640 x 640, dense, even batch): windows with pad tokens (Twp != Tw), non-square maps, padding masks, odd batches, images
that start in the middle of a 128-row tile. Plain data and the arithmetic that goes with it; importable without a GPU.

Every case has two distinct images (`valid`: their unpadded sizes, None = dense), tiled to fill the batch: slot k holds image k % 2."""
from collections import namedtuple

import numpy as np
import torch

Case = namedtuple("Case", "id size H W valid B dtype seed Tw Twp Tp rows")

#        id       size      H    W    valid sizes of the two images   B   dtype     seed   Tw  Twp   Tp   rows
CASES = [
    Case("s320", "small", 320, 320, None, 30, "float16", 5101, 25, 28, 448, 13440),
    Case("s384p", "small", 384, 320, ((384, 320), (256, 320)), 26, "bfloat16", 5102, 30, 32, 512, 13312),
    Case("t704", "tiny", 704, 704, None, 7, "float16", 5103, 121, 124, 1984, 13888),
    Case("t192", "tiny", 192, 256, None, 68, "float16", 5104, 12, 12, 192, 13056),
    Case("m448p", "medium", 448, 512, ((448, 512), (320, 384)), 16, "bfloat16", 5105, 56, 56, 896, 14336),
    Case("l384p", "large", 384, 320, ((384, 320), (256, 320)), 26, "float16", 5106, 30, 32, 512, 13312),
    Case("s640o", "small", 640, 640, None, 9, "float16", 5107, 100, 100, 1600, 14400),
    Case("s960", "small", 960, 960, None, 4, "float16", 5108, 225, 228, 3648, 14592),
    # C = 192 takes lwdetr_mlp_fused in float32 from 12800 rows (no block kernel, no chains in float32)
    Case("s320f", "small", 320, 320, ((320, 320), (256, 192)), 30, "float32", 5109, 25, 28, 448, 13440),
]
BY_ID = {c.id: c for c in CASES}
SENTINEL_CASES = ("s320", "s384p", "l384p", "t704")     # (d) nothing depends on what the buffers held
PADSTATE_CASES = ("s384p", "l384p")                     # (e) padding state of a cached plan
ARENA_CASES = ("s320", "l384p")                         # (f) LWDETR_ARENA=1
RATIO = 1.5                                             # ours <= RATIO x the reference's own 16-bit error (tests/test_gpu_baseline_configs.py)
F32_BOUNDS = {"front": 2e-4, "back": 5e-4}              # test_fp32_stages_match_oracle: memory / class_max, decoder layers / outputs


def dtype_of(case):
    return getattr(torch, case.dtype)


def case_images(case, seed=None, swap=False):
    """(images (2,3,H,W) f32 with the padded areas zeroed, mask (2,H,W) bool or None) of the case's two distinct images - as helpers.case_batch builds
    a golden batch. ``seed``: other pixels; ``swap``: the two valid sizes exchanged."""
    from lwdetr_amd.synth import synth_images
    x = synth_images(2, case.H, case.W, seed=case.seed if seed is None else seed)
    if case.valid is None:
        return x, None
    mask = torch.ones(2, case.H, case.W, dtype=torch.bool)
    valid = case.valid[::-1] if swap else case.valid
    for i, (h, w) in enumerate(valid):
        x[i, :, h:, :] = 0
        x[i, :, :, w:] = 0
        mask[i, :h, :w] = False
    return x, mask


def tile(t, B):
    """(2, ...) -> (B, ...): slot k holds element k % 2."""
    return None if t is None else t.repeat((B + 1) // 2, *([1] * (t.dim() - 1)))[:B].contiguous()


def winmajor_rows(hp, wp, twp):
    """Rows of one image's (16 * twp)-row window-major token block that hold real tokens, in the oracle's token order (its ``vit.block{i}`` is
    (B, 16 * h * w, C): window by window, h * w raster tokens each, no pad rows): row = window * twp + token."""
    tw = (hp // 4) * (wp // 4)
    return (np.arange(16)[:, None] * twp + np.arange(tw)[None, :]).reshape(-1)


def plan_geometry(size, H, W):
    """ForwardPlan's shape arithmetic restated (engine.py, ForwardPlan.__init__): Tw, Twp, Tp, level sizes, level start rows, S, nq."""
    import lwdetr_amd
    cfg = lwdetr_amd.get_args(size)
    scale = {"P3": 2.0, "P4": 1.0, "P5": 0.5}
    hp, wp = H // 16, W // 16
    tw = (hp // 4) * (wp // 4)
    twp = (tw + 3) // 4 * 4
    level_hw = [(int(hp * scale[s]), int(wp * scale[s])) for s in cfg.projector_scale]
    lsi = [0]
    for a, b in level_hw[:-1]:
        lsi.append(lsi[-1] + a * b)
    depth = cfg.vit_encoder_num_layers
    return dict(Hp=hp, Wp=wp, Tw=tw, Twp=twp, Tp=16 * twp, level_hw=level_hw, lsi=lsi, S=sum(a * b for a, b in level_hw), nq=cfg.num_queries,
                taps=sorted(i if i >= 0 else i + depth for i in cfg.out_feature_indexes), nl=cfg.dec_layers, d=cfg.hidden_dim)


# ---- the comparator of (b): one flat {name: (n_images, ...) float array} per side
def oracle_tensors(ref, col, geo):
    """The compared tensors out of helpers.oracle_lowp's result + collect (numpy, one entry per distinct image)."""
    t = {f"vit.block{i}": col[f"vit.block{i}"] for i in geo["taps"]}
    t["memory"], t["enc.class_max"] = col["memory"], col["enc.class_max"]
    for li in range(geo["nl"]):
        t[f"hs{li}"] = col[f"dec.layer{li}"]
    t["pred_logits"], t["pred_boxes"] = ref["pred_logits"], ref["pred_boxes"]
    for j in range(geo["nl"] - 1):
        t[f"aux{j}_logits"], t[f"aux{j}_boxes"] = ref["aux_logits"][:, j], ref["aux_boxes"][:, j]
    t["enc_logits"], t["enc_boxes"] = ref["enc_logits"], ref["enc_boxes"]
    return t


def plan_tensors(out, col, geo, C):
    """The same tensors out of one model call (output dict + _collect) as float32 numpy, one entry per batch slot; the taps at real tokens only, in the
    oracle's order (winmajor_rows)."""
    f = lambda v: v.float().cpu().numpy()
    B = out["pred_logits"].shape[0]
    rows = winmajor_rows(geo["Hp"], geo["Wp"], geo["Twp"])
    taps = f(col["taps_cat"]).reshape(B, geo["Tp"], len(geo["taps"]) * C)[:, rows]
    t = {f"vit.block{i}": taps[:, :, j * C:(j + 1) * C] for j, i in enumerate(geo["taps"])}
    t["memory"], t["enc.class_max"] = f(col["memory"]), f(col["enc.class_max"])
    hs = f(col["hs"]).reshape(geo["nl"], B, geo["nq"], geo["d"])
    for li in range(geo["nl"]):
        t[f"hs{li}"] = hs[li]
    t["pred_logits"], t["pred_boxes"] = f(out["pred_logits"]), f(out["pred_boxes"])
    for j, a in enumerate(out["aux_outputs"]):
        t[f"aux{j}_logits"], t[f"aux{j}_boxes"] = f(a["pred_logits"]), f(a["pred_boxes"])
    t["enc_logits"], t["enc_boxes"] = f(out["enc_outputs"]["pred_logits"]), f(out["enc_outputs"]["pred_boxes"])
    return t


def yardstick(t32, t16):
    """{tensor: {"max": (n,), "mean": (n,)}}: per distinct image, what the reference's own arithmetic costs in the 16-bit dtype."""
    y = {}
    for k in t32:
        e = np.abs(t16[k].astype(np.float64) - t32[k].astype(np.float64)).reshape(t32[k].shape[0], -1)
        y[k] = {"max": e.max(1), "mean": e.mean(1)}
    return y


def ratios(ours, t32, yard):
    """Per tensor, the worst ratio over the batch slots of max / mean |ours - fp32| to the yardstick of the slot's image (slot k holds image k % n):
    {tensor: {"max": r, "mean": r, "slot_max": k, "slot_mean": k, "ours_max": worst |err|, "ref_max": yardstick there}}."""
    res = {}
    for k, ref in t32.items():
        n = ref.shape[0]
        a = ours[k].astype(np.float64)
        img = np.arange(a.shape[0]) % n
        e = np.abs(a - ref.astype(np.float64)[img]).reshape(a.shape[0], -1)
        rmax = e.max(1) / np.maximum(yard[k]["max"][img], 1e-30)
        rmean = e.mean(1) / np.maximum(yard[k]["mean"][img], 1e-30)
        smax, smean = int(rmax.argmax()), int(rmean.argmax())
        res[k] = {"max": float(rmax[smax]), "mean": float(rmean[smean]), "slot_max": smax, "slot_mean": smean,
                  "ours_max": float(e.max(1)[smax]), "ref_max": float(yard[k]["max"][img][smax])}
    return res


def worst(r):
    """(largest ratio, tensor, column) of a ``ratios`` result."""
    return max((v[c], k, c) for k, v in r.items() for c in ("max", "mean"))
