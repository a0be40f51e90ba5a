"""Helper of tests/test_gpu_cocoeval.py: ONE rank under ``python -m torch.distributed.run --nproc-per-node 1``. Initialises the ``nccl``
(= RCCL) backend through lwdetr_amd.dist.init_from_env as an N-rank job does, then runs the native COCO evaluator on the generated set of
tests/cocoeval_cases.py twice: once with the process group hidden from it (no collective) and once as is, where
synchronize_between_processes gathers the per-detection records with tensor collectives. Both must give the same eval arrays, and those of
the oracle. Prints one line starting with COCOEVAL-RCCL-OK on success."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def run(ds, batches, dev):
    import lwdetr_amd
    ev = lwdetr_amd.CocoEvaluator(ds, ("bbox",))
    for ids, packed in batches:
        ev.update_packed(ids, torch.from_numpy(packed).to(dev))
    ev.synchronize_between_processes()
    ev.accumulate()
    return ev


def main():
    import cocoeval_cases as CS
    import cocoeval_ref as R
    from lwdetr_amd import dist as D
    rank, world, local = D.init_from_env()
    assert (rank, world) == (0, 1) and dist.is_initialized() and dist.get_backend() == "nccl", (rank, world, dist.get_backend())
    dev = torch.device("cuda", local)
    g = CS.generated()
    ref, _ = CS.oracle_run(R, g["dataset"], g["evaluated"])
    real = dist.is_initialized
    dist.is_initialized = lambda: False
    try:
        alone = run(g["dataset"], g["batches"], dev)
    finally:
        dist.is_initialized = real
    gathered = run(g["dataset"], g["batches"], dev)
    assert alone.collectives_run == 0 and gathered.collectives_run == 1
    for name in ("precision", "recall", "scores", "npig"):
        a, b = alone.coco_eval["bbox"].eval[name], gathered.coco_eval["bbox"].eval[name]
        assert np.array_equal(a, b), name
        if name != "npig":
            assert np.array_equal(b, ref.eval[name]), name
    assert np.array_equal(gathered.coco_eval["bbox"].stats, ref.stats)
    assert gathered.coco_eval["bbox"].params.imgIds == alone.coco_eval["bbox"].params.imgIds == sorted(CS.IMG_IDS[:7])
    print(f"COCOEVAL-RCCL-OK backend={dist.get_backend()} detections={gathered.sorted_store.cat.numel()} "
          f"AP={gathered.coco_eval['bbox'].stats[0]:.6f}", flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
