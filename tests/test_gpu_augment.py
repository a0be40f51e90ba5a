"""GPU: the training-time input transform (csrc/augment.hip through lwdetr_amd.augment.TrainTransform) against the reference's outputs
over real Pillow (tests/golden/augment.npz) and against the numpy restatement of the staged algorithm (tests/augment_ref.py, itself pinned
to the goldens by tests/test_augment_host.py). Everything is compared exactly: integer resampling, table-driven normalisation."""
import ctypes
import hashlib
import random

import numpy as np
import pytest
import torch

import augment_ref as A
from lwdetr_amd import _native
from lwdetr_amd.augment import AugmentParams, TrainTransform, convert_coco, make_coco_transforms, make_coco_transforms_square_div_64
from lwdetr_amd.models.nested import NestedTensor
from lwdetr_amd.preprocess import SquareResizeNormalize

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_CACHE = {}


def gold():
    if "gold" not in _CACHE:
        g, cases = A.load_cases()
        _CACHE["gold"] = (torch.from_numpy(g["lut"]), cases)
    return _CACHE["gold"]


def transform(dtype=torch.float32):
    if dtype not in _CACHE:
        _CACHE[dtype] = TrainTransform(dtype=dtype, device=DEV)
    return _CACHE[dtype]


def no_target(im):
    return convert_coco([], int(im.shape[1]), int(im.shape[0]), 0)


def run(images, params, dtype=torch.float32, targets=None):
    images = [torch.from_numpy(im) if isinstance(im, np.ndarray) else im for im in images]
    nt, tg = transform(dtype)(images, targets if targets is not None else [no_target(im) for im in images], params)
    assert isinstance(nt, NestedTensor) and nt.tensors.dtype == dtype and nt.mask.dtype == torch.bool
    return nt.tensors.cpu(), nt.mask.cpu(), tg


def check_targets(tg, case):
    assert set(tg) == set(A.TARGET_KEYS)
    for k in A.TARGET_KEYS:
        assert tg[k].device == DEV and tg[k].dtype == case.target[k].dtype and torch.equal(tg[k].cpu(), case.target[k]), (case.name, k)


def test_every_golden_case_alone_and_as_one_mixed_batch():
    table, cases = gold()
    small = [c for c in cases if c.out is not None]
    assert len(small) >= 20
    for c in small:
        out, mask, tg = run([c.image], [c.sample()], targets=[convert_coco(c.annotations, c.image.shape[1], c.image.shape[0], c.image_id)])
        exp, exp_mask = A.expected_batch([c.out], table)
        assert out.shape == exp.shape and torch.equal(out, exp) and torch.equal(mask, exp_mask) and not mask.any(), c.name
        check_targets(tg[0], c)
    params = [c.sample() for c in small]
    targets = [convert_coco(c.annotations, c.image.shape[1], c.image.shape[0], c.image_id) for c in small]
    out, mask, tg = run([c.image for c in small], params, targets=targets)
    exp, exp_mask = A.expected_batch([c.out for c in small], table)
    assert out.shape == exp.shape and torch.equal(out, exp), "mixed batch"
    assert torch.equal(mask, exp_mask) and mask.any()
    for i, c in enumerate(small):                                   # the padding, spelled out: zeros, mask True exactly there
        oh, ow = c.out_shape
        assert not out[i, :, oh:, :].any() and not out[i, :, :, ow:].any() and mask[i, oh:, :].all() and mask[i, :, ow:].all()
        assert not mask[i, :oh, :ow].any()
        check_targets(tg[i], c)
    _CACHE["mixed"] = (small, params, out)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16_bit_outputs_are_the_f32_result_cast(dtype):
    if "mixed" not in _CACHE:
        test_every_golden_case_alone_and_as_one_mixed_batch()
    small, params, out32 = _CACHE["mixed"]
    out, mask, _ = run([c.image for c in small], params, dtype)
    assert torch.equal(out, out32.to(dtype))


def test_default_parameter_cases_by_digest_and_subsample():
    table, cases = gold()
    big = [c for c in cases if c.out is None]
    assert {c.name for c in big} == {"default_square_branch2", "default_aspect_branch2"}
    out, mask, tg = run([c.image for c in big], [c.sample() for c in big],
                        targets=[convert_coco(c.annotations, c.image.shape[1], c.image.shape[0], c.image_id) for c in big])
    for i, c in enumerate(big):
        oh, ow = c.out_shape
        u8 = A.recover_u8(out[i, :, :oh, :ow], table)
        assert np.array_equal(u8[::A.SUB[0], ::A.SUB[1]], c.out_sub), c.name
        assert hashlib.sha256(np.ascontiguousarray(u8).tobytes()).hexdigest() == c.out_sha256, c.name
        assert not mask[i, :oh, :ow].any() and mask[i, oh:].all() and mask[i, :, ow:].all()
        check_targets(tg[i], c)


def test_sampling_inside_the_call_gives_the_reference_batch():
    """params=None: the transform draws, under the caller's seeds, what the reference's Compose draws - the acceptance check of the feature."""
    table, cases = gold()
    for name, make in (("residues_cw1_ow2", make_coco_transforms_square_div_64), ("aspect_branch2_flip", make_coco_transforms)):
        c = next(x for x in cases if x.name == name)
        recipe = {k: v for k, v in c.recipe.items() if k != "square"}
        t = make("train", dtype=torch.float32, device=DEV, **recipe)
        random.seed(c.seed)
        torch.manual_seed(c.seed)
        nt, tg = t([torch.from_numpy(c.image)], [convert_coco(c.annotations, c.image.shape[1], c.image.shape[0], c.image_id)])
        exp, exp_mask = A.expected_batch([c.out], table)
        assert torch.equal(nt.tensors.cpu(), exp) and torch.equal(nt.mask.cpu(), exp_mask)
        check_targets(tg[0], c)
    assert isinstance(make_coco_transforms("val", device=DEV), SquareResizeNormalize)
    assert isinstance(make_coco_transforms_square_div_64("val_speed", device=DEV), SquareResizeNormalize)


# (H, W, extra source row bytes, flip, resize1, crop (top, left, ch, cw), out_size): every alignment of the first pixel a lane reads
# (left % 4, flipped and not), of the row pitch (pitch % 4), every tail length (cw % 4, ow % 4), and each pass skipped alone and together.
SHAPES = [
    (20, 24, 0, False, None, None, (20, 24)),                      # nothing to do at all: bytes through the table, aligned 4-pixel loads
    (20, 23, 0, True, None, None, (20, 23)),                       # ... flipped, odd pitch
    (20, 24, 0, True, None, None, (31, 24)),                       # pass 4 alone reads the flipped source (pass 3 skipped)
    (20, 24, 0, False, None, None, (20, 37)),                      # pass 3 alone; pass 4 copies
    (21, 26, 1, True, None, None, (33, 41)),                       # passes 3 + 4, pitch % 4 == 1
    (21, 27, 2, False, None, (2, 1, 17, 20), (17, 20)),            # crop of the source only: left % 4 == 1, pitch % 4 == 3
    (21, 27, 3, True, None, (1, 2, 18, 21), (18, 21)),             # ... flipped, left % 4 == 2, tail 1
    (21, 28, 0, True, None, (0, 3, 21, 22), (29, 22)),             # pass 4 reads the flipped source window at left % 4 == 3, tail 2
    (21, 28, 0, False, None, (3, 4, 15, 23), (15, 30)),            # pass 3 reads the source window, tail 3 in, 2 out
    (30, 24, 0, True, (19, 24), (2, 1, 15, 20), (15, 20)),         # pass 2 alone reads the flipped source at left % 4 == 1 (pass 1 skipped)
    (30, 25, 1, False, (19, 25), (0, 2, 19, 21), (19, 21)),        # ... not flipped, left % 4 == 2, pitch % 4 == 0 through the padding
    (30, 26, 0, True, (45, 26), (7, 3, 30, 22), (30, 22)),         # ... upscale (3 taps), left % 4 == 3
    (30, 27, 0, False, (13, 27), (1, 4, 11, 23), (11, 23)),        # ... more than 2x down (many taps), left % 4 == 0, tail 3
    (22, 40, 0, True, (22, 29), (3, 5, 16, 19), (16, 19)),         # pass 1 alone (pass 2 skipped: A holds the window's rows), cw % 4 == 3
    (22, 40, 2, False, (22, 61), (0, 9, 22, 45), (22, 45)),        # ... upscale, cw % 4 == 1
    (35, 41, 0, True, (23, 29), (2, 3, 18, 21), (18, 21)),         # passes 1 + 2, cw % 4 == 1
    (35, 41, 0, False, (23, 29), (5, 7, 18, 22), (18, 22)),        # ... cw % 4 == 2 (rows of A and B start unaligned)
    (35, 41, 1, True, (50, 57), (30, 33, 20, 24), (20, 24)),       # ... upscale, window in the far corner, cw % 4 == 0
    (35, 41, 0, False, (23, 29), (2, 3, 18, 21), (26, 21)),        # passes 1 + 2 + 4 (pass 3 skipped): pass 4 reads B, odd width
    (35, 41, 0, True, (23, 29), (2, 3, 18, 21), (18, 33)),         # passes 1 + 2 + 3 (pass 4 copies C)
    (35, 41, 3, True, (23, 29), (2, 3, 18, 21), (27, 34)),         # all four passes, ow % 4 == 2
    (35, 41, 0, False, (23, 29), (0, 0, 23, 29), (31, 35)),        # all four, full window, ow % 4 == 3
    (22, 40, 0, True, (22, 29), (3, 5, 16, 19), (24, 28)),         # passes 1 + 3 + 4: pass 3 reads A
    (30, 26, 0, False, (45, 26), (7, 3, 30, 22), (36, 25)),        # passes 2 + 3 + 4: pass 3 reads B
    (9, 1030, 0, True, (10, 1029), (1, 2, 7, 1026), (8, 1027)),    # more than one block of lanes along x in every pass
    (3, 3000, 0, True, (3, 200), (0, 1, 3, 198), (3, 198)),        # pass 1 reducing by 15: the taps of 198 pixels do not fit the staged span
    (3, 3001, 0, False, None, None, (3, 200)),                     # ... pass 3, reading the source
]


def strided(img, extra):
    """The image as a device view whose rows are ``extra`` bytes further apart than its pixels need."""
    h, w = img.shape[:2]
    buf = torch.zeros(h, w * 3 + extra, dtype=torch.uint8, device=DEV)
    buf[:, :w * 3] = torch.from_numpy(img).to(DEV).view(h, w * 3)
    view = buf.as_strided((h, w, 3), (w * 3 + extra, 3, 1))
    assert view.stride(0) == w * 3 + extra
    return view


@pytest.mark.parametrize("idx", range(len(SHAPES)))
def test_shape_sweep_against_the_numpy_restatement(idx):
    h, w, extra, flip, resize1, crop, out_size = SHAPES[idx]
    img = A.synth_image(h, w, 300 + idx)
    p = AugmentParams(flip, resize1, crop, out_size)
    out, mask, _ = run([strided(img, extra)], [p])
    exp, exp_mask = A.expected_batch([A.augment_params_u8(img, p)], A.lut_f32())
    assert out.shape == exp.shape and torch.equal(out, exp) and torch.equal(mask, exp_mask)
    _CACHE.setdefault("sweep", {})[idx] = (img, p, exp[0])


def test_shape_sweep_as_one_batch_on_a_canvas_with_an_odd_width():
    """All the sweep's shapes together (mixed passes per launch, padding on every side of the alignment cases), twice on one stream."""
    items = []
    for idx, (h, w, extra, flip, resize1, crop, out_size) in enumerate(s for s in SHAPES if s[1] < 100):
        img = A.synth_image(h, w, 300 + idx)
        items.append((img, AugmentParams(flip, resize1, crop, out_size), extra))
    u8 = [A.augment_params_u8(img, p) for img, p, _ in items]
    exp, exp_mask = A.expected_batch(u8, A.lut_f32())
    assert exp.shape[-1] % 2 == 1
    t = transform()
    imgs = [strided(img, extra) for img, _, extra in items]
    tg = [no_target(im) for im in imgs]
    first, _ = t(imgs, tg, [p for _, p, _ in items])
    second, _ = t(imgs, tg, [p for _, p, _ in items])           # back to back: scratch and descriptors of the first call stay alive
    torch.cuda.synchronize()
    assert torch.equal(first.tensors.cpu(), exp) and torch.equal(first.mask.cpu(), exp_mask)
    assert torch.equal(second.tensors.cpu(), exp) and torch.equal(second.mask.cpu(), exp_mask)
    assert first.tensors.data_ptr() != second.tensors.data_ptr()


def test_empty_batch_no_stage_1_batch_host_and_non_contiguous_inputs():
    t = transform()
    nt, tg = t([], [])
    assert nt.tensors.shape == (0, 3, 0, 0) and nt.mask.shape == (0, 0, 0) and tg == []
    imgs = [A.synth_image(33, 47, 1), A.synth_image(40, 31, 2), A.synth_image(25, 25, 3)]
    params = [AugmentParams(True, None, None, (48, 56)), AugmentParams(False, None, None, (56, 48)), AugmentParams(True, None, None, (25, 25))]
    exp, exp_mask = A.expected_batch([A.augment_params_u8(im, p) for im, p in zip(imgs, params)], A.lut_f32())
    out, mask, _ = run(imgs, params)                                             # host tensors, no image has a stage 1
    assert torch.equal(out, exp) and torch.equal(mask, exp_mask)
    out, mask, _ = run([torch.from_numpy(im).to(DEV) for im in imgs], params)    # device tensors
    assert torch.equal(out, exp) and torch.equal(mask, exp_mask)
    chw = [torch.from_numpy(np.ascontiguousarray(im.transpose(2, 0, 1))).to(DEV).permute(1, 2, 0) for im in imgs]
    assert not chw[0].is_contiguous()
    out, mask, _ = run(chw, params)                                              # made contiguous inside, as SquareResizeNormalize does
    assert torch.equal(out, exp) and torch.equal(mask, exp_mask)


def test_bad_arguments_are_refused_through_the_abi_before_any_launch():
    t = TrainTransform(dtype=torch.float32, device=DEV)              # its own tables: this image's are the last in the buffer
    img = torch.from_numpy(A.synth_image(35, 41, 9)).to(DEV)
    p = AugmentParams(True, (23, 29), (2, 3, 18, 21), (27, 34))
    descs, scratch_bytes, hc, wc = t.describe([img], [p])
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, hc, wc), 7.0, device=DEV)
    mask = torch.full((1, hc, wc), 1, dtype=torch.uint8, device=DEV)
    raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    fn = _native.lib().lwdetr_augment_normalize
    base = dict(host=ctypes.addressof(descs), dev=raw.data_ptr(), b=1, tab=t._tables.buf.data_ptr(), tab_len=t._tables.buf.numel(),
                scratch=scratch.data_ptr(), scratch_bytes=scratch.numel(), lut=t.lut.data_ptr(), out=out.data_ptr(), mask=mask.data_ptr(),
                hc=hc, wc=wc, dtype=0)

    def call(**kw):
        a = dict(base, **kw)
        with torch.cuda.device(DEV):
            return fn(a["host"], a["dev"], a["b"], a["tab"], a["tab_len"], a["scratch"], a["scratch_bytes"], a["lut"], a["out"], a["mask"],
                      a["hc"], a["wc"], a["dtype"], _native.stream_ptr(DEV))

    bad = -1
    for key in ("host", "dev", "tab", "scratch", "lut", "out", "mask"):
        assert call(**{key: None}) == bad, key
    assert call(b=-1) == bad and call(hc=hc - 1) == bad and call(wc=wc - 1) == bad and call(hc=70000) == bad
    assert call(scratch_bytes=scratch_bytes - 16) == bad             # (each intermediate's size is rounded up to 16 bytes)
    assert call(tab_len=t._tables.length - 1) == bad
    assert call(dtype=3) == -2
    d = descs[0]
    for field, value in (("top", 6), ("left", 9), ("top", -1), ("left", -1), ("ch", 0), ("cw", 0), ("ch", 22), ("cw", 27), ("h1", 0), ("w1", 70000),
                         ("oh", 0), ("ow", wc + 1), ("height", 0), ("width", 70000), ("row_stride", 3 * 41 - 1), ("src", None), ("rows", 0),
                         ("row0", 35), ("rows", 36)):
        keep = getattr(d, field)
        setattr(d, field, value)
        assert call() == bad, (field, value)
        setattr(d, field, keep)
    assert call(b=0) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (mask == 1).all()                  # nothing above launched anything
    assert call() == 0
    torch.cuda.synchronize()
    exp, exp_mask = A.expected_batch([A.augment_params_u8(img.cpu().numpy(), p)], A.lut_f32())
    assert torch.equal(out.cpu(), exp) and torch.equal(mask.cpu().bool(), exp_mask)


def test_fresh_draws_on_a_cache_that_grows_stay_exact():
    """Every call draws new length pairs, as training does: the table buffer is replaced by larger ones while earlier launches are in
    flight, earlier pairs stay valid at their offsets, and the pixels stay exact."""
    from lwdetr_amd.augment import _AxisTables
    t = TrainTransform(dtype=torch.float32, device=DEV, scales=(48, 56, 64), resize_sizes=(40, 50, 60), crop_range=(38, 60))
    t._tables = _AxisTables(DEV, capacity=4096)
    assert t.prebuild() == 23 * 3 - 2
    imgs = [A.synth_image(57, 49, 1), A.synth_image(44, 71, 2), A.synth_image(66, 81, 3)]
    tg = [no_target(torch.from_numpy(im)) for im in imgs]
    first_ptr, results = t._tables.buf.data_ptr(), []
    for seed in range(6):
        random.seed(seed)
        torch.manual_seed(seed)
        params = [t.sample(im.shape[1], im.shape[0]) for im in imgs]
        nt, _ = t([torch.from_numpy(im) for im in imgs], tg, params)
        results.append((params, nt))
    assert t._tables.buf.data_ptr() != first_ptr and t._tables.buf.numel() > 4096
    for params, nt in results:
        exp, exp_mask = A.expected_batch([A.augment_params_u8(im, p) for im, p in zip(imgs, params)], A.lut_f32())
        assert torch.equal(nt.tensors.cpu(), exp) and torch.equal(nt.mask.cpu(), exp_mask)
