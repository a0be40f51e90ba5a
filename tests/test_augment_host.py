"""CPU: the host side of the training-time input transform (lwdetr_amd/augment.py) against tests/golden/augment.npz - the reference's
transforms over real Pillow (tools/gen_golden_augment.py) - and the ABI of lwdetr_augment_normalize. The numpy restatement of the staged,
crop-window algorithm (tests/augment_ref.py) is pinned to the reference's pixels here, before a GPU is involved."""
import ctypes
import hashlib
import os
import random
import re
import subprocess

import numpy as np
import pytest
import torch

import augment_ref as A
from helpers import ROOT


@pytest.fixture(scope="module")
def gold():
    return A.load_cases()


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from lwdetr_amd import _native
    return _native


def test_fixture_covers_the_cases_it_is_there_for(gold):
    _, cases = gold
    p = {c.name: c.sample() for c in cases}
    src = {c.name: c.image.shape[:2] for c in cases}
    assert p["flip_odd_width_branch1"].flip and p["flip_odd_width_branch1"].resize1 is None and src["flip_odd_width_branch1"][1] % 2 == 1
    assert not p["noflip_odd_width_branch1"].flip
    assert p["branch2_stage1_upscale"].resize1[0] > src["branch2_stage1_upscale"][0]
    assert src["branch2_stage1_downscale_3x"][0] > 2 * p["branch2_stage1_downscale_3x"].resize1[0]
    assert p["branch2_stage1_identity_left_odd"].resize1 == src["branch2_stage1_identity_left_odd"] and p["branch2_stage1_identity_left_odd"].crop[1] % 2 == 1
    assert p["crop_at_origin"].crop[:2] == (0, 0)
    q = p["crop_at_far_corner"]
    assert (q.crop[0] + q.crop[2], q.crop[1] + q.crop[3]) == q.resize1
    assert p["crop_is_full_image_no_randint"].crop == (0, 0) + p["crop_is_full_image_no_randint"].resize1
    assert p["cw_equals_ow_flip"].flip and p["cw_equals_ow_flip"].crop[3] == p["cw_equals_ow_flip"].out_size[1]
    assert p["ch_equals_oh"].crop[2] == p["ch_equals_oh"].out_size[0]
    assert p["stage2_nothing_to_do"].crop[2:] == p["stage2_nothing_to_do"].out_size
    assert p["branch1_width_equals_scale_flip"].flip and p["branch1_width_equals_scale_flip"].out_size[1] == src["branch1_width_equals_scale_flip"][1]
    res = {(v.crop[3] % 4, v.out_size[1] % 4) for k, v in p.items() if k.startswith("residues_")}
    assert {r[0] for r in res} == {0, 1, 2, 3} and {r[1] for r in res} == {0, 1, 2, 3}
    assert p["aspect_branch1_max_size_binds"].out_size == (26, 78)              # 64 would give 193 > max_size 80: round(80 * 40 / 121) = 26
    assert {c.name for c in cases if not c.square} >= {"aspect_branch1_max_size_binds", "aspect_branch2_flip", "default_aspect_branch2"}
    by = {c.name: c for c in cases}
    assert by["crop_removes_all_boxes"].converted["boxes"].shape[0] == 1 and by["crop_removes_all_boxes"].target["boxes"].shape[0] == 0
    c = by["crop_clips_a_box_to_zero_width"]
    zero_width = A.clipped_to_zero_width(c.converted["boxes"], p[c.name], c.image.shape[:2])
    assert zero_width >= 1 and 0 < c.target["boxes"].shape[0] <= c.converted["boxes"].shape[0] - zero_width
    assert by["no_annotations"].annotations == [] and by["no_annotations"].target["boxes"].shape == (0, 4)


def test_numpy_restatement_reproduces_every_reference_output(gold):
    """Sampled parameters + the crop-window, pass-skipping algorithm == the reference's Compose over Pillow, byte for byte."""
    _, cases = gold
    for c in cases:
        p = c.sample()
        out = A.augment_params_u8(c.image, p)
        assert out.shape[:2] == c.out_shape == tuple(p.out_size), c.name
        assert hashlib.sha256(out.tobytes()).hexdigest() == c.out_sha256, c.name
        assert np.array_equal(out[::A.SUB[0], ::A.SUB[1]], c.out_sub), c.name
        if c.out is not None:
            assert np.array_equal(out, c.out), c.name


def test_restatement_window_equals_resize_then_crop():
    """The restriction of stage 1 to the crop window is exact: the same bytes as resizing the whole image and cropping."""
    from oracle.preprocess_ref import _resample_axis
    img = A.synth_image(37, 53, 5)
    full = _resample_axis(_resample_axis(img[:, ::-1], 41, 1), 29, 0)
    win = A.augment_u8(img, True, (29, 41), (3, 5, 20, 30), (20, 30))
    assert np.array_equal(win, full[3:23, 5:35])


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def test_sampled_parameters_and_targets_equal_the_reference(gold):
    from lwdetr_amd.augment import convert_coco, transform_target
    _, cases = gold
    for c in cases:
        h, w = c.image.shape[:2]
        conv = convert_coco(c.annotations, w, h, c.image_id)
        assert set(conv) == set(A.TARGET_KEYS)
        for k in A.TARGET_KEYS:
            assert _same(conv[k], c.converted[k]), (c.name, k, conv[k], c.converted[k])
        tgt = transform_target(conv, c.sample(), (h, w))
        assert set(tgt) == set(A.TARGET_KEYS)
        for k in A.TARGET_KEYS:
            assert _same(tgt[k], c.target[k]), (c.name, k, tgt[k], c.target[k])
        assert tgt["boxes"].shape[0] == tgt["labels"].shape[0] == tgt["area"].shape[0] == tgt["iscrowd"].shape[0]
        assert all(torch.equal(conv[k], c.converted[k]) for k in A.TARGET_KEYS), "transform_target changed its input"


def test_draw_order_leaves_the_generators_where_the_reference_leaves_them():
    """Two images in a row under one seed: the second image's parameters depend on every draw the first one made (python's generator and
    torch's), so a missing or surplus draw shows. The crop that equals the image draws no offsets."""
    from lwdetr_amd.augment import sample_train_params
    random.seed(55)
    torch.manual_seed(55)
    state = torch.random.get_rng_state()
    p = sample_train_params(58, 45, scales=(48, 96), resize_sizes=(40,), crop_range=(40, 60))
    assert p.crop == (0, 0, 40, 51) and torch.equal(torch.random.get_rng_state(), state)       # the fixture's full-image crop: no torch draw
    random.seed(3)
    torch.manual_seed(3)
    state = torch.random.get_rng_state()
    a = sample_train_params(81, 66, scales=(62,), resize_sizes=(40, 50, 60), crop_range=(38, 60))
    assert a.crop is not None and a.crop[2:] != a.resize1 and not torch.equal(torch.random.get_rng_state(), state)
    rnd = random.Random(7)
    torch.manual_seed(7)
    b = sample_train_params(640, 480, rng=rnd)
    random.seed(7)
    torch.manual_seed(7)
    assert sample_train_params(640, 480) == b                                                  # rng= replaces the module-level generator
    sq, asp = sample_train_params(640, 480, rng=random.Random(1)), sample_train_params(640, 480, square=False, rng=random.Random(1))
    assert sq.out_size[0] == sq.out_size[1] and sq.out_size[0] % 64 == 0 and 448 <= sq.out_size[0] <= 896
    assert max(asp.out_size) <= 1333 and asp.out_size[0] != asp.out_size[1]


def test_lookup_table_equals_the_references(gold):
    from lwdetr_amd.augment import TrainTransform
    g, _ = gold
    ref = torch.from_numpy(g["lut"])
    assert ref.shape == (3, 256) and ref.dtype == torch.float32
    assert torch.equal(TrainTransform(dtype=torch.float32, device="cpu").lut, ref)
    assert torch.equal(A.lut_f32(), ref)


def test_value_errors():
    from lwdetr_amd.augment import AugmentParams, TrainTransform, convert_coco, make_coco_transforms, make_coco_transforms_square_div_64
    t = TrainTransform(dtype=torch.float32, device="cpu")
    img = torch.zeros(40, 50, 3, dtype=torch.uint8)
    tgt = convert_coco([], 50, 40, 1)
    ok = AugmentParams(False, None, None, (48, 48))
    for bad in (torch.zeros(40, 50, 3), torch.zeros(40, 50, dtype=torch.uint8), torch.zeros(40, 50, 4, dtype=torch.uint8),
                torch.zeros(3, 40, 50, dtype=torch.uint8), torch.zeros(0, 50, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            t([bad], [tgt], [ok])
    for params in (AugmentParams(False, (40, 50), (0, 11, 40, 40), (48, 48)), AugmentParams(False, (40, 50), (1, 0, 40, 40), (48, 48)),
                   AugmentParams(True, (40, 50), (-1, 0, 20, 20), (48, 48)), AugmentParams(False, (40, 50), (0, 0, 0, 20), (48, 48)),
                   AugmentParams(False, None, (0, 0, 41, 50), (48, 48)), AugmentParams(False, None, None, (0, 48)),
                   AugmentParams(False, (0, 50), None, (48, 48)), AugmentParams(False, None, None, (48, 70000))):
        with pytest.raises(ValueError):
            t([img], [tgt], [params])
    with pytest.raises(ValueError):
        t([img, img], [tgt], [ok, ok])
    with pytest.raises(ValueError):
        t([img], [tgt], [ok, ok])
    with pytest.raises(ValueError):
        t([img], None)
    with pytest.raises(ValueError):
        make_coco_transforms("test", device="cpu")
    with pytest.raises(ValueError):
        make_coco_transforms_square_div_64("trainval", device="cpu")
    assert make_coco_transforms("train", device="cpu").recipe["square"] is False
    assert make_coco_transforms_square_div_64("train", device="cpu").recipe["square"] is True


def test_lazy_export():
    import lwdetr_amd
    assert lwdetr_amd.augment.TrainTransform is __import__("lwdetr_amd.augment", fromlist=["x"]).TrainTransform


def test_descriptor_mirror_has_the_compilers_layout(built, tmp_path):
    from lwdetr_amd.augment import AugmentImage
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "lwdetr_hip.h"\nint main(){\nprintf("%zu", sizeof(lwdetr_augment_image));\n'
           + "".join(f'printf(" %zu", offsetof(lwdetr_augment_image, {f[0]}));\n' for f in AugmentImage._fields_)
           + 'printf(" %zu %zu %zu %zu\\n", sizeof(((lwdetr_augment_image*)0)->bounds_off), sizeof(((lwdetr_augment_image*)0)->coef_off), '
             'sizeof(((lwdetr_augment_image*)0)->ksize), sizeof(((lwdetr_augment_image*)0)->scratch_off));return 0;}\n')
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    ln = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    n = len(AugmentImage._fields_)
    assert ln[0] == ctypes.sizeof(AugmentImage)
    assert ln[1:1 + n] == [getattr(AugmentImage, f[0]).offset for f in AugmentImage._fields_]
    assert ln[1 + n:] == [getattr(AugmentImage, f).size for f in ("bounds_off", "coef_off", "ksize", "scratch_off")]


def test_symbol_is_declared_exported_and_bound(built):
    hdr = open(os.path.join(ROOT, "include", "lwdetr_hip.h")).read()
    assert re.search(r"\bint\s+lwdetr_augment_normalize\s*\(", hdr)
    assert hasattr(ctypes.CDLL(built.LIB_PATH), "lwdetr_augment_normalize")
    fn = built.lib().lwdetr_augment_normalize
    vp, i, lg = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert fn.argtypes == [vp, vp, i, vp, lg, vp, lg, vp, vp, vp, i, i, i, vp] and fn.restype is ctypes.c_int
    decl = re.search(r"int\s+lwdetr_augment_normalize\s*\(([^;]*)\)\s*;", hdr).group(1)
    assert len(decl.split(",")) == len(fn.argtypes)


def test_table_cache_grows_in_place_of_dropping_and_prebuild_covers_the_square_recipe():
    """A full buffer is replaced by a larger one that takes the content over: every (in, out) pair met so far stays resident at its offset.
    prebuild() leaves every stage-2 pair of the square recipe resident, so a fresh draw builds none of them."""
    from lwdetr_amd.augment import TrainTransform, _AxisTables
    from lwdetr_amd.preprocess import resample_tables
    tabs = _AxisTables(torch.device("cpu"), capacity=2048)
    pairs = [(40 + k, 64 + 3 * k) for k in range(12)]
    for k, pr in enumerate(pairs):
        tabs.require([pr, pairs[0]])
        assert set(tabs.entries) == set(pairs[:k + 1])
    assert tabs.buf.numel() > 2048 and tabs.length <= tabs.buf.numel()
    for pr in pairs:
        bo, co, ks, bounds = tabs.entries[pr]
        rb, rc = resample_tables(*pr)
        assert ks == rc.shape[1] and np.array_equal(bounds, rb)
        assert np.array_equal(tabs.buf[bo:bo + rb.size].numpy().reshape(rb.shape), rb)
        assert np.array_equal(tabs.buf[co:co + rc.size].numpy().reshape(rc.shape), rc)
    small = _AxisTables(torch.device("cpu"), capacity=512, limit=2000)              # at the limit the cache starts over with the batch at hand
    small.require(pairs[:2])
    small.require(pairs[2:6])
    assert set(small.entries) == set(pairs[2:6]) and small.length <= small.buf.numel()
    t = TrainTransform(dtype=torch.float32, device="cpu", scales=(48, 56, 64), resize_sizes=(50, 60), crop_range=(44, 50))
    assert t.prebuild() == 7 * 3 - 1 and (48, 48) not in t._tables.entries            # 44 ... 50 x three scales, less the skipped pass
    before = dict(t._tables.entries)
    for seed in range(40):
        random.seed(seed)
        torch.manual_seed(seed)
        p = t.sample(70, 90)
        if p.crop is not None:
            assert all(pr in before for pr in ((p.crop[3], p.out_size[1]), (p.crop[2], p.out_size[0])) if pr[0] != pr[1]), p
    assert TrainTransform(dtype=torch.float32, device="cpu", square=False).prebuild() == 0
