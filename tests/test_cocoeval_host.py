"""CPU: the COCO box evaluator without a GPU - hand-derived cases, the oracle (tests/cocoeval_ref.py) against the host instantiation of the
matching kernel (lwdetr_cocoeval_match_host: the kernel's per-(image, category) code with the lanes emulated) on a generated set that holds
every trap of COCOeval's rules, and the error paths. The curves run on the GPU only; tests/test_gpu_cocoeval.py repeats the hand-derived
cases through the whole native pipeline."""
import ctypes

import numpy as np
import pytest
import torch

import lwdetr_amd
import cocoeval_cases as CS
import cocoeval_ref as R
from lwdetr_amd import coco_eval as CE


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge
    ge.build()
    from lwdetr_amd import _native
    return _native


@pytest.fixture(scope="module")
def gen():
    g = CS.generated()
    g["ref"], g["table"] = CS.oracle_run(R, g["dataset"], g["evaluated"])
    return g


def host_table(ds, batches):
    """lwdetr_cocoeval_match_host over the batches, flattened slot by slot like the oracle's results list."""
    gt = CE.CocoGroundTruth(ds)
    outs = [CE.match_host(gt, ids, packed) for ids, packed in batches]
    return {k: np.concatenate([o[k].reshape(-1) for o in outs]) for k in outs[0]}


def assert_host_equals_oracle(ds, batches):
    ref, (cat, rank, matched, ignored) = CS.oracle_run(R, ds, batches)
    got = host_table(ds, batches)
    assert np.array_equal(got["cat"], cat) and np.array_equal(got["rank"], rank)
    assert np.array_equal(got["matched"], matched) and np.array_equal(got["ignored"], ignored)
    return ref


def close_to(stats, expected):
    """-1 and recall entries exactly; AP entries that are means of 1 / (1 + eps) = 0.9999999999999998 within 1e-12 of the literal."""
    return all((e == s) if e in (-1, 0) else abs(s - e) < 1e-12 for s, e in zip(stats, expected))


# ------------------------------------------------------------------------------------------------------------------ hand-derived
def test_perfect_detections(built):
    """Two gts (20x20 = 400: small; 50x50 = 2500: medium), each with its own box as detection. Every threshold matches (IoU 1), so in every
    populated group tp = [1], fp = [0]: rc = [1], pr = 1 / (1 + eps) = 0.9999999999999998 (COCOeval's eps keeps AP a hair under 1), found
    for all 101 recall thresholds; recall = 1. No gt is large: those entries stay -1."""
    ds, ids, packed = CS.hand_cases()["perfect"]
    ref = assert_host_equals_oracle(ds, [(ids, packed)])
    assert CS.AP1 == 0.9999999999999998
    assert close_to(ref.stats, [1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1]) and list(ref.stats[6:]) == [1, 1, 1, 1, 1, -1]
    p = ref.eval["precision"]
    assert (p[:, :, :, 3, :] == -1).all() and (p[:, :, 0, 1, :] == CS.AP1).all() and (p[:, :, 1, 2, :] == CS.AP1).all()


def test_lower_scored_detection_is_the_true_positive_at_iou_50_only(built):
    """gt [0,0,10,20] (area 200, small). A (score .9) is far away; B (score .8) = [0,0,10,10]: IoU = 100 / (100 + 200 - 100) = 0.5 exactly.
    At t = 0.5 the test `iou < t` is false, B matches: tp = [0,1], fp = [1,1], rc = [0,1], pr = [0, 1/(2+eps)] = [0, .5] -> running maximum
    [.5, .5] -> precision .5 at all 101 recall thresholds: AP50 = 0.5. At the nine other thresholds nothing matches: rc = [0,0], precision 0
    (recall threshold 0 finds index 0, the others none). AP = 0.5 / 10 = 0.05 = AP small, AP75 = 0. maxDets = 1 sees only A: AR1 = 0;
    AR10 = AR100 = AR small = (1 + 9 * 0) / 10 = 0.1. No medium or large gt: -1."""
    ds, ids, packed = CS.hand_cases()["second_is_tp_at_50"]
    ref = assert_host_equals_oracle(ds, [(ids, packed)])
    assert list(ref.stats) == [0.05, 0.5, 0.0, 0.05, -1, -1, 0.0, 0.1, 0.1, 0.1, -1, -1]
    got = host_table(ds, [(ids, packed)])
    at50 = [1 << (a * 10) for a in range(4)]
    assert list(got["matched"][:2]) == [0, sum(at50)]        # B: threshold 0.5 only; in medium / large it takes the gt as an ignored one
    assert got["ignored"][1] & sum(at50) == at50[2] + at50[3]
    assert list(got["rank"][:2]) == [0, 1]


def test_crowd_gt_absorbs_three_detections(built):
    """A crowd gt [0,0,100,100] and a plain gt [200,200,50,50] (2500: medium). Three detections (scores .9 .8 .7) lie inside the crowd: their
    IoU with it is i / da = 1, they all match it (a crowd stays available after a match) and are ignored, not false positives. The fourth
    (.6) is the plain gt's box: the only counted detection, a true positive: AP = AP50 = AP75 = AP medium = 1 / (1 + eps), AR10 = AR100 =
    AR medium = 1. maxDets = 1 keeps only the top detection, which is ignored: AR1 = 0. The crowd counts in no npig: small and large are -1."""
    ds, ids, packed = CS.hand_cases()["crowd_absorbs_three"]
    ref = assert_host_equals_oracle(ds, [(ids, packed)])
    assert close_to(ref.stats, [1, 1, 1, -1, 1, -1, 0, 1, 1, -1, 1, -1]) and list(ref.stats[6:]) == [0, 1, 1, -1, 1, -1]
    got = host_table(ds, [(ids, packed)])
    every = (1 << 40) - 1
    assert list(got["matched"][:4]) == [every] * 4 and list(got["ignored"][:3]) == [every] * 3
    assert got["ignored"][3] == sum(1 << (a * 10 + t) for a in (1, 3) for t in range(10))      # the plain gt is outside small and large


def test_gt_of_area_exactly_1024_is_small_and_medium(built):
    """One 32x32 gt (area 1024.0) with its own box as detection: [0, 1024] and [1024, 9216] both hold it (inclusive ends), so small and
    medium are 1 / (1 + eps) and 1; large has no gt: -1."""
    ds, ids, packed = CS.hand_cases()["area_1024"]
    ref = assert_host_equals_oracle(ds, [(ids, packed)])
    assert close_to(ref.stats, [1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1]) and list(ref.stats[6:]) == [1, 1, 1, 1, 1, -1]
    assert list(ref.npig[0]) == [1, 1, 1, 0]


# ------------------------------------------------------------------------------------------------------------------ generated set
def test_generated_set_holds_every_trap(gen):
    """A generator change cannot silently drop a trap: each one is looked for in the oracle's own intermediate data."""
    ref, ds = gen["ref"], gen["dataset"]
    packed = np.concatenate([p.reshape(-1, 6) for _, p in gen["evaluated"]])
    img_of = np.concatenate([np.repeat(ids, p.shape[1]) for ids, p in gen["evaluated"]])
    scores, labels = packed[:, 0], packed[:, 1]
    valid = np.isin(labels, CS.CAT_IDS)
    # equal scores inside an image and across images (same category)
    seen_in, seen_across = False, False
    for c in CS.CAT_IDS:
        sel = labels == c
        for s in np.unique(scores[sel]):
            imgs = img_of[sel & (scores == s)]
            seen_in |= len(imgs) != len(set(imgs))
            seen_across |= len(set(imgs)) > 1
    assert seen_in and seen_across
    ious = [m for m in ref.ious.values() if len(m)]
    assert any(np.isin(m, R.IOU_THRS).any() for m in ious)                                     # an IoU exactly equal to a threshold
    assert any(((row >= .5).sum() >= 2 and len(set(row[row >= .5])) < (row >= .5).sum()) for m in ious for row in m)   # two gts, equal IoU
    brk = False                                                                                # a non-ignored match followed by ignored gts
    for (img, cat), m in ref.ious.items():
        if len(m):
            ig = np.array([g["ignore"] for g in ref.gts[img, cat]])
            brk |= bool(((m[:, ig == 0] >= .5).any(1) & (m[:, ig == 1] >= .5).any(1)).any()) if ig.any() and (ig == 0).any() else False
    assert brk
    _, _, matched, ignored = gen["table"]
    large = sum(1 << (30 + t) for t in range(10))
    assert ((matched & large) == 0)[(ignored & large) == large].any()                          # unmatched and outside the area range
    gt_cats = {a["category_id"] for a in ds["annotations"]}
    assert 7 in gt_cats and not (labels == 7).any() and (labels == 8).any() and 8 not in gt_cats
    k8 = CS.CAT_IDS.index(8)
    assert (ref.eval["precision"][:, :, k8] == -1).all() and (ref.npig[k8] == 0).all()          # a category with no gts at all
    assert 99 in ref.img_ids_all and 99 not in ref.img_ids                                     # an image that is never updated
    ids = [i for b, _ in gen["batches"] for i in b]
    assert len(ids) == len(set(ids)) + 1                                                       # one duplicate update
    assert (~valid).sum() >= 4 and (labels[~valid] != -1).any()                                # labels outside the category list
    w, h = packed[:, 4] - packed[:, 2], packed[:, 5] - packed[:, 3]
    assert (valid & (w == 0)).any() and (valid & (w < 0) & (h < 0)).any()                      # zero-area and inverted boxes
    assert any(len(v) > 100 for v in ref.dts.values())                                         # maxDet truncation
    assert any(a["area"] == 1024 for a in ds["annotations"]) and any("ignore" in a for a in ds["annotations"])


def test_host_kernel_equals_the_oracle_on_the_generated_set(built, gen):
    """Order, ranks and the 40-bit matched / ignored masks of every detection slot, bit for bit."""
    cat, rank, matched, ignored = gen["table"]
    got = host_table(gen["dataset"], gen["evaluated"])
    assert np.array_equal(got["cat"], cat)
    assert np.array_equal(got["rank"], rank)
    assert np.array_equal(got["matched"], matched)
    assert np.array_equal(got["ignored"], ignored)
    assert (rank >= 0).sum() == (cat >= 0).sum() and rank.max() == 99 and (cat >= 0).sum() < len(cat)


def test_host_kernel_terminates_on_non_finite_boxes_and_scores(built, gen):
    """Every loop's trip count is fixed by the counts: NaN / inf records return, and still equal the oracle."""
    ids, packed = gen["evaluated"][0]
    packed = packed.copy()
    packed[0, 0, 2:] = np.nan
    packed[0, 1, 4] = np.inf
    packed[0, 2, 0] = np.nan
    packed[1, 3, 2] = -np.inf
    assert_host_equals_oracle(gen["dataset"], [(ids, packed)])


# ------------------------------------------------------------------------------------------------------------------ error paths
def test_first_occurrence_keeps_the_first_of_every_value():
    keys = torch.tensor([5, 3, 5, 9, 3, 3, 7])
    assert CE.first_occurrence(keys).tolist() == [True, True, False, True, False, False, True]
    assert CE.first_occurrence(torch.zeros(0, dtype=torch.int64)).tolist() == []
    assert CE.first_occurrence(torch.tensor([4])).tolist() == [True]


def test_score_order_key_orders_like_the_mergesort_of_negated_scores():
    score = torch.tensor([0.5, float("nan"), -0.0, 0.0, 1.0, float("-inf"), 0.5, float("inf")])
    cat = torch.zeros(8, dtype=torch.int64)
    order = torch.sort(CE.score_order_key(cat, score), stable=True).indices.tolist()
    assert order == np.argsort(-score.numpy().astype(np.float64), kind="mergesort").tolist()
    both = torch.sort(CE.score_order_key(torch.tensor([1, 0, 1, 0]), torch.tensor([.9, .1, .95, .2])), stable=True).indices.tolist()
    assert both == [3, 1, 2, 0]


def test_constructor_and_update_error_paths(built, tmp_path):
    ds, ids, packed = CS.hand_cases()["perfect"]
    with pytest.raises(NotImplementedError):
        lwdetr_amd.CocoEvaluator(ds, ("segm",))
    with pytest.raises(NotImplementedError):
        lwdetr_amd.CocoEvaluator(ds, ["bbox", "keypoints"])
    with pytest.raises(ValueError):
        lwdetr_amd.CocoEvaluator(ds, ("boxes",))
    with pytest.raises(TypeError):
        lwdetr_amd.CocoGroundTruth(17)
    ev = lwdetr_amd.CocoEvaluator(ds, ("bbox",))
    with pytest.raises(ValueError, match="not in the ground truth"):
        ev.update({12345: {"scores": torch.zeros(1), "labels": torch.zeros(1, dtype=torch.int64), "boxes": torch.zeros(1, 4)}})
    with pytest.raises(ValueError, match="not in the ground truth"):
        CE.match_host(ev.coco_gt, [2], packed)
    # the three accepted sources pack the same tables
    import json
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(ds))

    class Holder:
        dataset = ds
    for other in (lwdetr_amd.CocoGroundTruth(str(path)), lwdetr_amd.CocoGroundTruth(Holder())):
        assert np.array_equal(other.grp_off, ev.coco_gt.grp_off) and np.array_equal(other.box, ev.coco_gt.box)
    assert ev.coco_eval["bbox"].params.catIds == [1, 2] and ev.img_ids == []


def test_limits_are_refused_not_truncated(built):
    """Above 1024 detections per image, 256 annotations per (image, category) or 1024 categories: LWDETR_ERR_UNSUPPORTED from the entry,
    before anything runs; exactly at the limits the call goes through."""
    N = built
    many = CS.dataset([1], [1], [CS.ann(i + 1, 1, 1, [i, 0, 10, 10]) for i in range(N.COCOEVAL_MAX_GROUP + 1)])
    with pytest.raises(N.NativeError, match="unsupported"):
        CE.match_host(CE.CocoGroundTruth(many), [1], CS.pack([[(.9, 1, 0, 0, 10, 10)]]))
    many["annotations"].pop()
    out = CE.match_host(CE.CocoGroundTruth(many), [1], CS.pack([[(.9, 1, 255, 0, 265, 10)]]))
    assert out["matched"][0, 0] == (1 << 40) - 1 and out["ignored"][0, 0] == sum(1 << (a * 10 + t) for a in (2, 3) for t in range(10))
    ds = CS.hand_cases()["perfect"][0]
    gt = CE.CocoGroundTruth(ds)
    with pytest.raises(N.NativeError, match="unsupported"):
        CE.match_host(gt, [1], np.zeros((1, N.COCOEVAL_MAX_DETS + 1, 6), np.float32))
    assert CE.match_host(gt, [1], np.zeros((1, N.COCOEVAL_MAX_DETS, 6), np.float32))["cat"].max() == -1
    cats = CS.dataset([1], list(range(N.COCOEVAL_MAX_CATS + 1)), [])
    with pytest.raises(N.NativeError, match="unsupported"):
        CE.match_host(CE.CocoGroundTruth(cats), [1], CS.pack([[(.9, 1, 0, 0, 10, 10)]]))
    cats["categories"].pop()
    assert CE.match_host(CE.CocoGroundTruth(cats), [1], CS.pack([[(.9, 1, 0, 0, 10, 10)]]))["cat"][0, 0] == 1
    assert ctypes.sizeof(N.CocoGt) == 72
