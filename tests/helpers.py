"""Shared test utilities: golden loading, deterministic weights, key->shape tables, the GEMM launch-path record."""
import contextlib
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# (case name -> size, image dims) - must match oracle/gen_golden.py:CASES
CASES = {
    "tiny_640": ("tiny", [(640, 640)]),
    "small_640": ("small", [(640, 640), (640, 640)]),
    "medium_640": ("medium", [(640, 640)]),
    "large_640": ("large", [(640, 640)]),
    "xlarge_640": ("xlarge", [(640, 640)]),
    "xlarge_960": ("xlarge", [(960, 960)]),
    "tiny_192x256": ("tiny", [(192, 256), (192, 256)]),
    "small_padded": ("small", [(448, 512), (320, 384)]),
    "large_padded": ("large", [(384, 320), (256, 320)]),
}
MAX_SAMPLES = 4096


def sample_idx(n):
    if n <= MAX_SAMPLES:
        return np.arange(n)
    stride = -(-n // MAX_SAMPLES)
    stride += 1 - (stride % 2)
    return np.arange(0, n, stride)[:MAX_SAMPLES]


def load_golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False)


def golden_state_dict(g, seed=0):
    """Rebuild the synthetic state dict the golden was generated with, from the key/shape table it stores."""
    from lwdetr_amd.synth import synth_param
    sd = {}
    for k, s in zip(g["sd_keys"], g["sd_shapes"]):
        shape = tuple(int(x) for x in str(s).split(",") if x != "")
        sd[str(k)] = synth_param(str(k), shape, seed)
    return sd


def case_batch(name):
    """(size, padded images (B,3,H,W), mask (B,H,W) bool) for a golden case."""
    from lwdetr_amd.synth import synth_images
    size, dims = CASES[name]
    hmax, wmax = max(d[0] for d in dims), max(d[1] for d in dims)
    full = synth_images(len(dims), hmax, wmax, seed=1234)
    mask = torch.ones(len(dims), hmax, wmax, dtype=torch.bool)
    for i, (h, w) in enumerate(dims):
        full[i, :, h:, :] = 0
        full[i, :, :, w:] = 0
        mask[i, :h, :w] = False
    return size, full, mask


# ---- CPU oracle over a full BASELINE batch: images are independent, so the batch is cut into small chunks that worker
# processes (spawned: the parent may hold a GPU context) run side by side on the host cores.
def _oracle_chunk(job):
    size, seed, lo, hi, res, img_seed, threads, forced = job
    import torch as _t
    _t.set_num_threads(threads)
    import lwdetr_amd
    from lwdetr_amd.synth import synth_images, synth_state_dict
    from oracle import lwdetr_torch as O
    cfg = lwdetr_amd.get_args(size)
    model, _, _ = lwdetr_amd.build_model(cfg)
    sd = synth_state_dict(model.state_dict(), seed=seed)
    x = synth_images(hi, res, res, seed=img_seed)[lo:hi]          # counter-based generator: image i is the same in any batch
    col = {}
    with _t.no_grad():
        out = O.forward(sd, cfg, x, forced_topk=None if forced is None else _t.from_numpy(forced), collect=col)
        res_ = O.postprocess(out, _t.tensor([[480.0, 640.0]] * (hi - lo)), cfg.num_select)
        sc, lb, bx = (_t.stack([r[k] for r in res_]) for k in ("scores", "labels", "boxes"))
    return {"pred_logits": out["pred_logits"].numpy(), "pred_boxes": out["pred_boxes"].numpy(),
            "enc_logits": out["enc_outputs"]["pred_logits"].numpy(), "enc_boxes": out["enc_outputs"]["pred_boxes"].numpy(),
            "aux_logits": np.stack([a["pred_logits"].numpy() for a in out["aux_outputs"]], 1),
            "aux_boxes": np.stack([a["pred_boxes"].numpy() for a in out["aux_outputs"]], 1),
            "topk_idx": out["topk_idx"].numpy(), "enc_class_max": col["enc.class_max"].numpy(), "post_scores": sc.numpy(), "post_labels": lb.numpy(), "post_boxes": bx.numpy()}


def oracle_batch(size, batch, res, img_seed, seed=0, chunk=2, forced_topk=None):
    """fp32 CPU oracle outputs for synth_images(batch, res, res, img_seed) with synth weights `seed` (dict of numpy arrays).
    forced_topk (batch, nq) int64 numpy: two-stage indices to use instead of the oracle's own (teacher forcing)."""
    import multiprocessing as mp
    cores = len(os.sched_getaffinity(0))
    jobs_n = (batch + chunk - 1) // chunk
    procs = max(1, min(jobs_n, cores // 8))
    threads = max(1, min(16, cores // procs))
    jobs = [(size, seed, lo, min(lo + chunk, batch), res, img_seed, threads,
             None if forced_topk is None else np.ascontiguousarray(forced_topk[lo:min(lo + chunk, batch)]))
            for lo in range(0, batch, chunk)]
    if procs == 1:
        parts = [_oracle_chunk(j) for j in jobs]
    else:
        with mp.get_context("spawn").Pool(procs) as pool:
            parts = pool.map(_oracle_chunk, jobs)
    return {k: np.concatenate([p[k] for p in parts], 0) for k in parts[0]}


def _collect_numpy(col):
    """The oracle's collected stages as float32 numpy arrays (batch first), under the oracle's own names."""
    return {k: v.float().numpy() for k, v in col.items() if k.startswith(("vit.block", "dec.layer")) or k in ("memory", "enc.class_max")}


def _oracle_lowp_chunk(job):
    size, idx, res, img_seed, dtype_name, forced, seed, threads = job[:8]
    images, mask, want_col = job[8:] if len(job) > 8 else (None, None, False)
    import torch as _t
    _t.set_num_threads(threads)
    import lwdetr_amd
    from lwdetr_amd.synth import synth_images, synth_state_dict
    from oracle import lwdetr_torch as O
    dtype = getattr(_t, dtype_name)
    cfg = lwdetr_amd.get_args(size)
    model, _, _ = lwdetr_amd.build_model(cfg)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in synth_state_dict(model.state_dict(), seed=seed).items()}
    if images is None:
        x = synth_images(max(idx) + 1, res, res, seed=img_seed)[list(idx)].to(dtype)      # counter-based generator: image i is the same in any batch
    else:
        x = _t.from_numpy(images).to(dtype)
    m = None if mask is None else _t.from_numpy(mask)
    core = O.msda_core
    O.msda_core = lambda value, shapes, loc, aw: core(value.float(), shapes, loc.float(), aw.float()).to(value.dtype)
    try:
        col = {}
        with _t.no_grad():
            out = O.forward(sd, cfg, x, m, forced_topk=None if forced is None else _t.from_numpy(np.ascontiguousarray(forced)), collect=col)
    finally:
        O.msda_core = core
    f = lambda t: t.float().numpy()
    r = {"pred_logits": f(out["pred_logits"]), "pred_boxes": f(out["pred_boxes"]), "enc_class_max": f(col["enc.class_max"]),
         "enc_logits": f(out["enc_outputs"]["pred_logits"]), "enc_boxes": f(out["enc_outputs"]["pred_boxes"]),
         "aux_logits": np.stack([f(a["pred_logits"]) for a in out["aux_outputs"]], 1),
         "aux_boxes": np.stack([f(a["pred_boxes"]) for a in out["aux_outputs"]], 1)}
    if images is not None:
        r["topk_idx"] = out["topk_idx"].numpy()
    if want_col:
        r.update({"collect:" + k: v for k, v in _collect_numpy(col).items()})
    return r


def oracle_lowp(size, n, res, img_seed, dtype, forced_topk, seed=0, threads=16, idx=None, chunk=2, images=None, mask=None, collect=None):
    """The reference arithmetic IN A 16-BIT DTYPE on the CPU: oracle/lwdetr_torch.py with every parameter
    and the input cast to ``dtype`` - each torch op then rounds its result to that dtype, as the reference does under
    ``model.half()`` / bfloat16 - for images ``idx`` (default: the first ``n``) of synth_images(., res, res, img_seed), with the
    two-stage selection forced (``forced_topk`` is indexed with the same ``idx``). The deformable sampling core runs in float32 on
    the 16-bit value / location / weight tensors (CPU grid_sample returns NaN in half precision; the reference's own path casts
    there too, models/transformer.py:356). Images are independent: chunks of ``chunk`` images run in worker processes side by side.
    Returns final + encoder (+ auxiliary) logits / boxes as float32 numpy arrays in the order of ``idx``: their distance to the
    fp32 oracle is what 16-bit arithmetic itself costs on this network - the yardstick for the HIP path's 16-bit error.

    ``images`` (n', 3, H, W) float32 (tensor or numpy), with ``mask`` (n', H, W) bool or None: run on these instead of the synthetic ones
    (``n``, ``res``, ``img_seed`` and ``idx`` are then unused, ``forced_topk`` (n', nq) goes with the images as given; None = the run's own
    selection, e.g. with ``dtype`` float32 for the oracle itself) - the result then carries ``topk_idx`` too. ``collect``: a dict that receives the
    oracle's collected stages (``memory``, ``enc.class_max``, ``vit.block{i}``, ``dec.layer{i}``) as float32 numpy arrays."""
    import multiprocessing as mp
    if images is None:
        idx = list(range(n)) if idx is None else [int(i) for i in idx]
    else:
        images = np.ascontiguousarray(images.numpy() if isinstance(images, torch.Tensor) else images, dtype=np.float32)
        mask = None if mask is None else np.ascontiguousarray(mask.numpy() if isinstance(mask, torch.Tensor) else mask, dtype=bool)
        idx = list(range(images.shape[0]))
    cores = len(os.sched_getaffinity(0))
    groups = [idx[i:i + chunk] for i in range(0, len(idx), chunk)]
    procs = max(1, min(len(groups), cores // 8))
    th = max(1, min(threads, cores // procs))
    name = str(dtype).split(".")[-1]
    fk = lambda g: None if forced_topk is None else np.ascontiguousarray(np.asarray(forced_topk)[g])
    if images is None and collect is None:
        jobs = [(size, g, res, img_seed, name, fk(g), seed, th) for g in groups]
    else:
        jobs = [(size, g, res, img_seed, name, fk(g), seed, th, None if images is None else images[g],
                 None if mask is None else mask[g], collect is not None) for g in groups]
    if procs == 1:
        parts = [_oracle_lowp_chunk(j) for j in jobs]
    else:
        with mp.get_context("spawn").Pool(procs) as pool:
            parts = pool.map(_oracle_lowp_chunk, jobs)
    res_ = {k: np.concatenate([p[k] for p in parts], 0) for k in parts[0]}
    if collect is not None:
        collect.update({k[len("collect:"):]: res_[k] for k in res_ if k.startswith("collect:")})
    return {k: v for k, v in res_.items() if not k.startswith("collect:")}


def _oracle_run_job(job):
    size, images, mask, dtype_name, forced, threads = job
    import torch as _t
    col = {}
    ref = oracle_lowp(size, 0, 0, 0, getattr(_t, dtype_name), forced, threads=threads, images=images, mask=mask, collect=col, chunk=len(images))
    return ref, col


def oracle_run(size, images, mask, dtype, forced_topk=None, threads=16):
    """oracle_lowp on explicit ``images`` / ``mask`` with its collected stages, in worker processes: (result, collect) of numpy arrays. ``dtype``
    float32 with ``forced_topk`` None is the fp32 oracle itself (its own two-stage selection, returned as ``topk_idx``); a 16-bit ``dtype`` with the
    oracle's selection forced is the yardstick. Workers are spawned (the parent may hold a GPU context and its own thread settings): images are
    independent, so one worker per image where the cores allow (16-bit CPU ops thread poorly)."""
    import multiprocessing as mp
    images = np.ascontiguousarray(images.numpy() if isinstance(images, torch.Tensor) else images, dtype=np.float32)
    mask = None if mask is None else np.ascontiguousarray(mask.numpy() if isinstance(mask, torch.Tensor) else mask, dtype=bool)
    forced_topk = None if forced_topk is None else np.ascontiguousarray(forced_topk)
    cores = len(os.sched_getaffinity(0))
    n = images.shape[0]
    procs = max(1, min(n, cores // 8))
    th = max(1, min(threads, cores // procs))
    name = str(dtype).split(".")[-1]
    parts = [slice(i, i + 1) for i in range(n)] if procs > 1 else [slice(0, n)]
    jobs = [(size, images[p], None if mask is None else mask[p], name, None if forced_topk is None else forced_topk[p], th) for p in parts]
    with mp.get_context("spawn").Pool(procs) as pool:
        res = pool.map(_oracle_run_job, jobs)
    return tuple({k: np.concatenate([r[j][k] for r in res], 0) for k in res[0][j]} for j in range(2))


def box_iou_xyxy(a, b):
    """(n,4) x (m,4) -> (n,m) IoU, numpy."""
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:], b[None, :, 2:])
    inter = np.clip(rb - lt, 0, None).prod(-1)
    aa = np.clip(a[:, 2:] - a[:, :2], 0, None).prod(-1)
    ab = np.clip(b[:, 2:] - b[:, :2], 0, None).prod(-1)
    return inter / np.maximum(aa[:, None] + ab[None, :] - inter, 1e-9)


@contextlib.contextmanager
def served_by(family, launches=1):
    """Asserts that the lwdetr_gemm / lwdetr_gemm_few launches inside the block went to exactly the kernel family `family` (a name of
    lwdetr_gemm_path_name: "gemm_dma_64x64_d3", "gemm_big_256_kb64", "gemm_pt", "gemm_few_conv_kch6", ...), `launches` times (None: at least
    once), and to no other."""
    import torch
    from lwdetr_amd import _native
    before = _native.gemm_path_counts()
    assert family in before, f"unknown GEMM kernel family {family!r}: {sorted(before)}"
    yield
    torch.cuda.synchronize()
    after = _native.gemm_path_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    if launches is None:
        assert set(delta) == {family}, f"expected launches of {family} only, the launches went to {delta}"
    else:
        assert delta == {family: launches}, f"expected {launches} launch(es) of {family}, the launches went to {delta}"


@contextlib.contextmanager
def vit_served_by(form, launches=1):
    """As served_by for the record of vitblock.hip (lwdetr_vit_path_counts): the lwdetr_vit_block / lwdetr_vit_qkv / lwdetr_vit_stem launches inside
    the block went to exactly the instantiation `form` (a name of lwdetr_vit_path_name: "vitblock_f16_c192_nh1_wpc2_qkv1_g16_1", "vit_qkv_bf16_c384",
    ...), `launches` times (None: at least once), and to no other."""
    import torch
    from lwdetr_amd import _native
    before = _native.vit_path_counts()
    assert form in before, f"unknown ViT kernel form {form!r}: {sorted(before)}"
    yield
    torch.cuda.synchronize()
    after = _native.vit_path_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    if launches is None:
        assert set(delta) == {form}, f"expected launches of {form} only, the launches went to {delta}"
    else:
        assert delta == {form: launches}, f"expected {launches} launch(es) of {form}, the launches went to {delta}"


@contextlib.contextmanager
def msda_served_by(form, launches=1):
    """As served_by for the record of msda.hip (lwdetr_msda_path_counts): the lwdetr_msda_forward / lwdetr_msda_backward / lwdetr_msda_fused_forward
    launches inside the block went to exactly the instantiation `form` (a name of lwdetr_msda_path_name: "msda_vec8_f16_pn", "msda_generic_f64",
    "msda_fused_bf16_l2p4", "msda_backward_f32", ...), `launches` times (None: at least once), and to no other."""
    import torch
    from lwdetr_amd import _native
    before = _native.msda_path_counts()
    assert form in before, f"unknown deformable-attention kernel form {form!r}: {sorted(before)}"
    yield
    torch.cuda.synchronize()
    after = _native.msda_path_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    if launches is None:
        assert set(delta) == {form}, f"expected launches of {form} only, the launches went to {delta}"
    else:
        assert delta == {form: launches}, f"expected {launches} launch(es) of {form}, the launches went to {delta}"


@contextlib.contextmanager
def attn_served_by(form, launches=1):
    """As served_by for the record of attention.hip (lwdetr_attn_path_counts): the lwdetr_attention launches inside the block went to exactly the
    instantiation `form` (a name of lwdetr_attn_path_name: "attn_wave_f16_hd16_qt2_short", "attn_win_bf16_hd32", "attn_ring_f16_hd64_q2w8u1", ...),
    `launches` times (None: at least once), and to no other."""
    import torch
    from lwdetr_amd import _native
    before = _native.attn_path_counts()
    assert form in before, f"unknown attention kernel form {form!r}: {sorted(before)}"
    yield
    torch.cuda.synchronize()
    after = _native.attn_path_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    if launches is None:
        assert set(delta) == {form}, f"expected launches of {form} only, the launches went to {delta}"
    else:
        assert delta == {form: launches}, f"expected {launches} launch(es) of {form}, the launches went to {delta}"


@contextlib.contextmanager
def mlp_served_by(form, launches=1):
    """As served_by for the record of mlp.hip (lwdetr_mlp_path_counts): the lwdetr_mlp_fused / lwdetr_vit_block_few / lwdetr_ffn_partial launches inside
    the block went to exactly the instantiation `form` (a name of lwdetr_mlp_path_name: "mlp_f16_c192_proj1_qkv1", "mlp_small_bf16_tt1_qkv0_frag1",
    "vit_few384_f16_qkv1", "ffn_bf16_c256", ...), `launches` times (None: at least once), and to no other."""
    import torch
    from lwdetr_amd import _native
    before = _native.mlp_path_counts()
    assert form in before, f"unknown MLP kernel form {form!r}: {sorted(before)}"
    yield
    torch.cuda.synchronize()
    after = _native.mlp_path_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    if launches is None:
        assert set(delta) == {form}, f"expected launches of {form} only, the launches went to {delta}"
    else:
        assert delta == {form: launches}, f"expected {launches} launch(es) of {form}, the launches went to {delta}"


@contextlib.contextmanager
def chain_served_by(form, launches=1):
    """As served_by for the record of chain.hip (lwdetr_chain_path_counts): the lwdetr_enc_chain / lwdetr_row_chain launches inside the block went to
    exactly the instantiation `form` (a name of lwdetr_chain_path_name: "enc_f16_d256_pf1_narrow", "row_bf16_d256_res1_q0", "split_f16_d384", ...),
    `launches` times (None: at least once), and to no other."""
    import torch
    from lwdetr_amd import _native
    before = _native.chain_path_counts()
    assert form in before, f"unknown chain kernel form {form!r}: {sorted(before)}"
    yield
    torch.cuda.synchronize()
    after = _native.chain_path_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    if launches is None:
        assert set(delta) == {form}, f"expected launches of {form} only, the launches went to {delta}"
    else:
        assert delta == {form: launches}, f"expected {launches} launch(es) of {form}, the launches went to {delta}"
