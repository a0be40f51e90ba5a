"""GPU: the native COCO box evaluator (csrc/cocoeval.hip through lwdetr_amd.CocoEvaluator) against the fp64 restatement of COCOeval in
tests/cocoeval_ref.py - per-detection masks and ranks, npig, precision / recall / scores / stats BIT FOR BIT (same operations, same order,
IEEE f64, contraction off: no tolerance anywhere in this file) - plus the hand-derived cases, input variations, determinism, graph capture,
the chunk carry of the curves kernel, the engine.evaluate calling sequence and one rank under the distributed launcher."""
import os

import numpy as np
import pytest
import torch

import lwdetr_amd
import lwdetr_amd.models
import cocoeval_cases as CS
import cocoeval_ref as R
from helpers import case_batch, golden_state_dict, load_golden
from lwdetr_amd import coco_eval as CE
from test_gpu_dist import _torchrun

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ARRAYS = ("precision", "recall", "scores")


@pytest.fixture(scope="module")
def gen():
    g = CS.generated()
    g["ref"], g["table"] = CS.oracle_run(R, g["dataset"], g["evaluated"])
    return g


def predictions(ids, packed, device=DEV, dtype=torch.float32):
    """The {image_id: {"scores", "labels", "boxes"}} dict of engine.py:144 from a (B, K, 6) record."""
    p = torch.from_numpy(np.asarray(packed))
    return {int(i): {"scores": p[b, :, 0].to(device=device, dtype=dtype), "labels": p[b, :, 1].to(device=device, dtype=torch.int64),
                     "boxes": p[b, :, 2:].to(device=device, dtype=dtype)} for b, i in enumerate(ids)}


def run(ds, batches, how="packed", **kw):
    ev = lwdetr_amd.CocoEvaluator(ds, ("bbox",))
    for ids, packed in batches:
        if how == "packed":
            ev.update_packed(ids, torch.from_numpy(packed).to(DEV))
        else:
            ev.update(predictions(ids, packed, **kw))
    ev.synchronize_between_processes()
    ev.accumulate()
    return ev


def device_table(ev, batches):
    outs = [[o.cpu().numpy().reshape(-1) for o in bt.out] for bt in ev._batches[:len(batches)]]
    return [np.concatenate([o[j] for o in outs]) for j in range(5)]


def assert_equals_oracle(ev, ref):
    e = ev.coco_eval["bbox"].eval
    assert np.array_equal(e["npig"], ref.npig)
    for name in ARRAYS:
        assert e[name].dtype == np.float64 and e[name].shape == ref.eval[name].shape
        assert np.array_equal(e[name], ref.eval[name]), name
    assert np.array_equal(ev.coco_eval["bbox"].stats, ref.stats)
    assert e["counts"] == ref.eval["counts"]


def same_eval(a, b):
    return all(np.array_equal(a.coco_eval["bbox"].eval[n], b.coco_eval["bbox"].eval[n]) for n in ARRAYS + ("npig",)) and \
        np.array_equal(a.coco_eval["bbox"].stats, b.coco_eval["bbox"].stats)


def close_to(stats, expected):
    return all((e == s) if e in (-1, 0) else abs(s - e) < 1e-12 for s, e in zip(stats, expected))


HAND = {   # derivations: the docstrings of tests/test_cocoeval_host.py; 1 stands for a mean of 1 / (1 + eps) in the six AP entries
    "perfect": [1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1],
    "second_is_tp_at_50": [0.05, 0.5, 0.0, 0.05, -1, -1, 0.0, 0.1, 0.1, 0.1, -1, -1],
    "crowd_absorbs_three": [1, 1, 1, -1, 1, -1, 0, 1, 1, -1, 1, -1],
    "area_1024": [1, 1, 1, 1, 1, -1, 1, 1, 1, 1, 1, -1],
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_derived_cases_through_the_native_pipeline(name, capsys):
    ds, ids, packed = CS.hand_cases()[name]
    ev = run(ds, [(ids, packed)])
    stats = ev.coco_eval["bbox"].stats
    assert isinstance(stats, np.ndarray) and stats.shape == (12,)
    assert close_to(stats, HAND[name]) and list(stats[6:]) == HAND[name][6:], stats
    if name == "second_is_tp_at_50":
        assert list(stats) == HAND[name]
    ref, _ = CS.oracle_run(R, ds, [(ids, packed)])
    assert_equals_oracle(ev, ref)
    ev.summarize()
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "IoU metric: bbox" and len(lines) == 13
    assert lines[1] == " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = {:0.3f}".format(stats[0])
    assert lines[12] == " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = {:0.3f}".format(stats[11])


def test_kernels_equal_the_oracle_on_the_generated_set(gen):
    """All four batches, the duplicate update of image 5 included (the first one wins): masks and ranks of every slot equal the oracle's and
    the host form's, npig exact, the curves bit for bit."""
    ev = run(gen["dataset"], gen["batches"])
    cat, rank, matched, ignored = gen["table"]
    got = device_table(ev, gen["evaluated"])
    assert np.array_equal(got[0], cat) and np.array_equal(got[2], rank)
    assert np.array_equal(got[3], matched) and np.array_equal(got[4], ignored)
    gt = CE.CocoGroundTruth(gen["dataset"])
    for (ids, packed), bt in zip(gen["batches"], ev._batches):
        host = CE.match_host(gt, ids, packed)
        for name, o in zip(("cat", "score", "rank", "matched", "ignored"), bt.out):
            assert np.array_equal(host[name], o.cpu().numpy()), name
    assert_equals_oracle(ev, gen["ref"])
    assert ev.coco_eval["bbox"].params.imgIds == sorted(CS.IMG_IDS[:7]) and 99 not in ev.img_ids
    assert sorted(set(int(i) for i in ev.img_ids)) == sorted(CS.IMG_IDS[:7]) and len(ev.img_ids) == 8


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_detections_from_half_precision_outputs(gen, dtype):
    """f16 / bf16 model outputs are just other f32 values: round the records, feed them in that dtype, compare with the oracle on the
    rounded values."""
    batches = []
    for ids, packed in gen["evaluated"]:
        r = packed.copy()
        r[:, :, [0, 2, 3, 4, 5]] = torch.from_numpy(packed[:, :, [0, 2, 3, 4, 5]]).to(dtype).float().numpy()
        batches.append((ids, r))
    ref, _ = CS.oracle_run(R, gen["dataset"], batches)
    ev = run(gen["dataset"], gen["evaluated"], how="update", dtype=dtype)
    assert_equals_oracle(ev, ref)


def test_update_forms_agree(gen):
    """update with device tensors, with host tensors, in one batch against many, and update_packed: identical eval arrays."""
    base = run(gen["dataset"], gen["batches"])
    assert same_eval(base, run(gen["dataset"], gen["batches"], how="update"))
    assert same_eval(base, run(gen["dataset"], gen["batches"], how="update", device="cpu"))
    (i0, p0), (i1, p1), big, dup = gen["batches"]
    merged = [(i0 + i1, np.concatenate([p0, p1])), big, dup]
    assert same_eval(base, run(gen["dataset"], merged))
    single = [([i], p[b:b + 1]) for ids, p in gen["batches"] for b, i in enumerate(ids)]
    assert same_eval(base, run(gen["dataset"], single, how="update"))
    ragged = lwdetr_amd.CocoEvaluator(gen["dataset"], ("bbox",))                 # images of 40 and of 130 detections in ONE dict
    pr = {}
    for ids, p in gen["evaluated"]:
        pr.update(predictions(ids, p))
    ragged.update(pr)
    ragged.accumulate()                                                          # accumulate synchronises when nobody did
    assert same_eval(base, ragged)


def test_two_full_runs_are_bit_identical(gen):
    a, b = run(gen["dataset"], gen["batches"]), run(gen["dataset"], gen["batches"])
    assert same_eval(a, b)
    for x, y in zip(a._batches, b._batches):
        assert all(torch.equal(p, q) for p, q in zip(x.out, y.out))
    assert all(torch.equal(getattr(a.sorted_store, n), getattr(b.sorted_store, n)) for n in ("cat", "score", "rank", "matched", "ignored"))


def test_update_packed_is_capturable_and_replays_bit_for_bit(gen):
    """No host synchronisation inside update_packed when the image ids are a device tensor: the call is captured with torch.cuda.graph on
    one stream; a replay on another batch written into the captured inputs reproduces that batch's eager outputs bit for bit."""
    (i0, p0), (i1, p1) = gen["batches"][:2]
    eager = lwdetr_amd.CocoEvaluator(gen["dataset"], ("bbox",))
    eager.update_packed(i0, torch.from_numpy(p0).to(DEV))
    eager.update_packed(i1, torch.from_numpy(p1).to(DEV))
    torch.cuda.synchronize()
    ev = lwdetr_amd.CocoEvaluator(eager.coco_gt, ("bbox",))
    ids = torch.tensor(i0, device=DEV)
    rec = torch.from_numpy(p0).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ev.update_packed(ids, rec)                                               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        ev.update_packed(ids, rec)
    captured = ev._batches[-1].out
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager._batches[0].out))
    ids.copy_(torch.tensor(i1, device=DEV))
    rec.copy_(torch.from_numpy(p1).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(captured, eager._batches[1].out))
    bad = lwdetr_amd.CocoEvaluator(eager.coco_gt, ("bbox",))                     # a device id the ground truth does not hold: deferred
    bad.update_packed(torch.tensor([11, 12345, 42], device=DEV), torch.from_numpy(p0).to(DEV))
    with pytest.raises(ValueError, match="not in the ground truth"):
        bad.synchronize_between_processes()


def test_segment_longer_than_a_chunk_carries(capsys):
    """One category, 40 images x 75 = 3 000 detections: twelve 256-chunks per group, so the running tp / fp counts, the recall look-ups and
    the running maximum all cross chunk borders."""
    ds, ids, packed = CS.carry_set()
    batches = [(ids[:20], packed[:20]), (ids[20:], packed[20:])]
    ref, _ = CS.oracle_run(R, ds, batches)
    ev = run(ds, batches)
    assert ev.sorted_store.cat.numel() > 2560 and (ref.eval["precision"][:, :, 0, 0, 2] > 0).any()
    assert_equals_oracle(ev, ref)


def test_evaluate_loop_with_the_native_evaluator(capsys):
    """The calling sequence of the reference's engine.evaluate (engine.py:93-164) as tests/test_gpu_model.py::test_evaluate_loop_contract walks
    it, with the native criterion, PostProcess and this evaluator together: tiny model, one 192x256 golden case, made-up ground truth built
    around the model's own detections. stats equal the oracle run on the same PostProcess output."""
    g = load_golden("tiny_192x256")
    size, images, mask = case_batch("tiny_192x256")
    args = lwdetr_amd.get_args(size)
    args.native_criterion = True
    model, criterion, postprocessors = lwdetr_amd.build_model(args)
    model.load_state_dict(golden_state_dict(g), strict=True)
    model = model.to(DEV).eval()
    criterion.eval()
    with torch.no_grad():
        probe = postprocessors["bbox"](model(lwdetr_amd.models.NestedTensor(images, mask).to(DEV)), torch.tensor([[480, 640]] * 2, device=DEV))
    anns, rng = [], np.random.RandomState(3)
    for image_id, res in zip((7, 9), probe):
        bx, lb = res["boxes"].float().cpu().numpy().astype(np.float64), res["labels"].cpu().numpy()
        for j in range(0, 24, 2):                                               # every other one of the top detections, jittered
            x0, y0, x1, y1 = bx[j] + rng.randint(-3, 4, size=4)
            anns.append(CS.ann(100 * image_id + j, image_id, int(lb[j]), [x0, y0, max(x1 - x0, 1.0), max(y1 - y0, 1.0)], iscrowd=int(j == 8)))
    base_ds = type("Coco", (), {"dataset": CS.dataset([7, 9, 11], list(range(91)), anns)})()
    targets_of = lambda i: {"labels": torch.tensor([a["category_id"] for a in anns if a["image_id"] == i]),
                            "boxes": torch.tensor([[.5, .5, .2, .2]] * sum(a["image_id"] == i for a in anns))}
    data_loader = [(lwdetr_amd.models.NestedTensor(images, mask),
                    [{"image_id": torch.tensor(7), "orig_size": torch.tensor([480, 640]), **targets_of(7)},
                     {"image_id": torch.tensor(9), "orig_size": torch.tensor([480, 640]), **targets_of(9)}])]
    iou_types = tuple(k for k in ("segm", "bbox") if k in postprocessors.keys())
    coco_evaluator = lwdetr_amd.CocoEvaluator(base_ds, iou_types)
    kept = {}
    for samples, targets in data_loader:
        samples = samples.to(DEV)
        targets = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
        outputs = model(samples)
        loss_dict = criterion(outputs, targets)
        assert all(torch.isfinite(v).all() for v in loss_dict.values())
        orig_target_sizes = torch.stack([t["orig_size"] for t in targets], dim=0)
        results = postprocessors["bbox"](outputs, orig_target_sizes)
        res = {target["image_id"].item(): output for target, output in zip(targets, results)}
        kept.update(res)
        if coco_evaluator is not None:
            coco_evaluator.update(res)
    coco_evaluator.synchronize_between_processes()
    coco_evaluator.accumulate()
    coco_evaluator.summarize()
    stats = coco_evaluator.coco_eval["bbox"].stats.tolist()
    assert len(stats) == 12 and len(capsys.readouterr().out.splitlines()) == 13
    packed = np.stack([torch.cat([kept[i]["scores"].float()[:, None], kept[i]["labels"].float()[:, None], kept[i]["boxes"].float()], 1)
                       .cpu().numpy() for i in (7, 9)])
    ref, _ = CS.oracle_run(R, base_ds.dataset, [([7, 9], packed)])
    assert_equals_oracle(coco_evaluator, ref)
    assert stats == ref.stats.tolist() and stats[1] > 0 and coco_evaluator.img_ids == [7, 9]


def test_one_rank_under_the_launcher_gathers_with_collectives():
    """synchronize_between_processes with torch.distributed initialised (nccl = RCCL, one rank): the collective runs and eval is what it
    is without it. A fresh child process with its own timeout."""
    r = _torchrun([os.path.join(os.path.dirname(os.path.abspath(__file__)), "cocoeval_one_rank_driver.py")], timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert any(ln.startswith("COCOEVAL-RCCL-OK") for ln in r.stdout.splitlines()), r.stdout[-2000:]
