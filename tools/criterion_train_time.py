"""Times the native training criterion (csrc/match.hip's cost launch + csrc/match_train.hip) beside two baselines on the same card:

    python tools/criterion_train_time.py [--batches 4,16] [--targets 7,40,100] [--form focal] [--dtype fp32] [--n 30]
Per (batch, targets per image), at 4 layers x 3900 queries x 91 classes, 13 groups, every image with that many synthetic targets:
  * native forward (no grad) and forward + backward: host clock around a call that ends in a device synchronise, median / min / max over
    --n calls after 3 warm-up calls;
  * the phase split by HIP events around each entry (cost, grouped assign, partials, finish, backward), median over --n rounds, and the
    solver's shortest-path step counts;
  * baseline "torch + scipy": what a user runs without this criterion - the reference's algorithm in f32 torch on the same device, the cost
    matrix copied to the host and scipy.optimize.linear_sum_assignment per (layer, group, image), losses by indexed scatters, gradients by
    autograd - forward and forward + backward, the same clock;
  * baseline "eval criterion": the existing evaluation criterion's four launches on ONE group's 300 queries of the same outputs (it
    refuses more than 1024 queries and more than one group): a floor for the part the two criteria share;
  * the largest relative distance of the native loss values to the baseline's at the timed size.
Written for profiles/r10a_criterion_train.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def stats(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="4,16")
    ap.add_argument("--targets", default="7,40,100")
    ap.add_argument("--form", default="focal", choices=["focal", "iabce", "varifocal", "possup"])
    ap.add_argument("--dtype", default="fp32", choices=["fp16", "bf16", "fp32"])
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--nq", type=int, default=3900)
    ap.add_argument("--groups", type=int, default=13)
    ap.add_argument("--rehearse", action="store_true", help="no GPU: run the torch + scipy baseline once on the CPU and stop")
    a = ap.parse_args()
    import numpy as np
    import torch
    import torch.nn.functional as F
    from scipy.optimize import linear_sum_assignment
    import lwdetr_amd
    import lwdetr_amd.models as M
    import criterion_ref as R
    import criterion_train_ref as TR
    from lwdetr_amd import _native
    from lwdetr_amd.models import criterion as NC
    T = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}[a.dtype]
    dev = torch.device("cpu" if a.rehearse else "cuda:0")
    nq, G, ncls, nl = a.nq, a.groups, 91, 4
    gw = nq // G
    lib = _native.lib()
    print(f"device {'cpu (rehearsal)' if a.rehearse else torch.cuda.get_device_name(0)}, torch {torch.__version__}, hip {torch.version.hip}; {nl} layers x {nq} queries x {ncls} classes, "
          f"{G} groups, form {a.form}, outputs {a.dtype}, n = {a.n}")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        out = []
        for _ in range(a.n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            out.append((time.perf_counter() - t0) * 1e3)
        return stats(out)

    def box_xyxy(x):
        cx, cy, w, h = x.unbind(-1)
        w, h = w.clamp(min=0), h.clamp(min=0)
        return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)

    def torch_criterion(layers, targets):
        """The reference's algorithm (matcher.py:50-111, lwdetr.py:256-506, train mode) in torch on the tensors' device, scipy on the host."""
        sizes = [len(t["labels"]) for t in targets]
        num_boxes = max(float(sum(sizes) * G), 1.0)
        tgt_ids, tgt_bbox = torch.cat([t["labels"] for t in targets]), torch.cat([t["boxes"] for t in targets])
        losses = {}
        for n, (lg, bx) in enumerate(layers):
            bs = lg.shape[0]
            with torch.no_grad():
                prob, ob = lg.flatten(0, 1).sigmoid(), bx.flatten(0, 1)
                giou = R.generalized_box_iou(box_xyxy(ob), box_xyxy(tgt_bbox))
                neg = 0.75 * (prob ** 2.0) * (-(1 - prob + 1e-8).log())
                pos = 0.25 * ((1 - prob) ** 2.0) * (-(prob + 1e-8).log())
                # the reference calls torch.cdist(p=1) here; on the (B nq) x sumT matrix of B = 16 with 40 or 100 targets it returned wrong
                # distances on the torch build this was first run with (profiles/r10a_criterion_train.txt), so the L1 cost is spelled out
                l1 = (ob[:, None, :] - tgt_bbox[None, :, :]).abs().sum(-1)
                cost = 5.0 * l1 + 2.0 * (pos[:, tgt_ids] - neg[:, tgt_ids]) + 2.0 * (-giou)
                cost = cost.view(bs, nq, -1).cpu()
                idx = None
                for g, cg in enumerate(cost.split(gw, dim=1)):
                    ig = [linear_sum_assignment(c[i]) for i, c in enumerate(cg.split(sizes, -1))]
                    idx = ig if idx is None else [(np.concatenate([p[0], q[0] + gw * g]), np.concatenate([p[1], q[1]])) for p, q in zip(idx, ig)]
            bi = torch.cat([torch.full((len(i),), b, dtype=torch.int64) for b, (i, _) in enumerate(idx)]).to(dev)
            qi = torch.cat([torch.as_tensor(i, dtype=torch.int64) for i, _ in idx]).to(dev)
            tj = [torch.as_tensor(j, dtype=torch.int64).to(dev) for _, j in idx]
            tcls = torch.cat([t["labels"][j] for t, j in zip(targets, tj)])
            tbox = torch.cat([t["boxes"][j] for t, j in zip(targets, tj)])
            src = bx[bi, qi]
            p = lg.sigmoid()
            ious = torch.diag(R.box_iou(box_xyxy(src.detach()), box_xyxy(tbox))[0]).detach()
            if a.form == "iabce":
                pw, nw = torch.zeros_like(lg), p ** 2
                t = (p[bi, qi, tcls].pow(0.25) * ious.pow(0.75)).clamp(min=0.01).detach()
                pw[bi, qi, tcls] = t
                nw = nw.index_put((bi, qi, tcls), 1 - t)
                ce = (-pw * p.log() - nw * (1 - p).log()).sum() / num_boxes
            else:
                tgt = torch.zeros_like(lg)
                tgt[bi, qi, tcls] = ious if a.form != "focal" else torch.ones_like(ious)
                if a.form == "possup":
                    tgt = tgt / (tgt.view(bs, -1, 1).amax(1, True) + 1e-8)
                bce = F.binary_cross_entropy_with_logits(lg, tgt, reduction="none")
                if a.form == "possup":
                    loss = (0.25 * (tgt > 0).float() + 0.75 * (tgt <= 0).float()) * bce * (torch.abs(tgt - p) ** 2)
                elif a.form == "varifocal":
                    loss = bce * (tgt * (tgt > 0).float() + 0.75 * (p - tgt).abs().pow(2) * (tgt <= 0).float())
                else:
                    p_t = p * tgt + (1 - p) * (1 - tgt)
                    loss = (0.25 * tgt + 0.75 * (1 - tgt)) * bce * ((1 - p_t) ** 2)
                ce = loss.mean(1).sum() / num_boxes * nq
            sfx = "" if n == 0 else ("_enc" if n == len(layers) - 1 else f"_{n - 1}")
            losses["loss_ce" + sfx] = ce
            losses["loss_bbox" + sfx] = (src - tbox).abs().sum() / num_boxes
            losses["loss_giou" + sfx] = (1 - torch.diag(R.generalized_box_iou(box_xyxy(src), box_xyxy(tbox)))).sum() / num_boxes
        return losses

    for b in [int(x) for x in a.batches.split(",")]:
        host = R.synth_outputs(nl, b, nq, ncls, 500 + b)
        for t in [int(x) for x in a.targets.split(",")]:
            targets = [{k: v.to(dev) for k, v in tg.items()} for tg in R.synth_targets((t,) * b, ncls, 500 + t)]
            for tg in targets:
                tg["boxes"] = tg["boxes"].float()
            leaves = [(lg.to(dev).to(T).requires_grad_(True), bx.to(dev).to(T).requires_grad_(True)) for lg, bx in host]
            plain = [(lg.detach(), bx.detach()) for lg, bx in leaves]
            crit = M.TrainSetCriterion(ncls, M.GroupHungarianMatcher(focal_alpha=0.25, **R.COST_W), {}, 0.25, ["labels", "boxes", "cardinality"],
                                       group_detr=G, **TR.FORM_FLAGS[a.form])
            print(f"\n== B = {b}, {t} targets per image ({nl * b * G} assignment problems of {gw} x {t}) ==")

            def native_fwd():
                with torch.no_grad():
                    return crit(R.as_outputs(plain), targets)

            def native_fb():
                losses = crit(R.as_outputs(leaves), targets)
                return torch.autograd.grad(sum(v for v in losses.values() if v.grad_fn is not None), [x for p in leaves for x in p])

            def torch_fwd():
                with torch.no_grad():
                    return torch_criterion(plain, targets)

            def torch_fb():
                losses = torch_criterion(leaves, targets)
                return torch.autograd.grad(sum(losses.values()), [x for p in leaves for x in p])

            if a.rehearse:
                print({k: round(v.item(), 6) for k, v in torch_fwd().items()}, [tuple(g.shape) for g in torch_fb()])
                continue
            res = {}
            for name, fn in (("native forward", native_fwd), ("native forward + backward", native_fb), ("torch + scipy forward", torch_fwd),
                             ("torch + scipy forward + backward", torch_fb)):
                res[name] = timed(fn)
                print(f"{name:36s} median {res[name][0]:9.3f} ms   min {res[name][1]:9.3f}   max {res[name][2]:9.3f}")
            print(f"forward speed-up {res['torch + scipy forward'][0] / res['native forward'][0]:.1f} x, forward + backward "
                  f"{res['torch + scipy forward + backward'][0] / res['native forward + backward'][0]:.1f} x")
            nat, ref = native_fwd(), torch_fwd()
            worst = max(abs(nat[k].item() - v.item()) / max(abs(v.item()), 1e-12) for k, v in ref.items())
            print(f"largest relative distance of a native loss value to the baseline's: {worst:.2e} ({len(ref)} keys)")
            gn, gt = native_fb(), torch_fb()
            gerr = max(((x.float() - y.float()).abs().max() / y.float().abs().max().clamp(min=1e-30)).item() for x, y in zip(gn, gt))
            print(f"largest gradient distance to the baseline's autograd, relative to the tensor's maximum: {gerr:.2e}")

            # phase split by events around the entries
            m = crit.matcher
            arr, keep = NC._layer_array(plain, True)
            packed = NC._Packed(targets, dev, nq, m._offsets)
            ws = m._match(arr, nl, keep[0], packed, G)
            out = torch.empty(nl, 5, dtype=torch.float32, device=dev)
            grads = [torch.empty_like(x) for x in keep]
            garr = (_native.CritLayer * nl)()
            for n in range(nl):
                garr[n].logits, garr[n].boxes = grads[2 * n].data_ptr(), grads[2 * n + 1].data_ptr()
            up = torch.ones(nl, 5, dtype=torch.float32, device=dev)
            st, dt, form = _native.stream_ptr(dev), _native.dtype_code(T), TR.FORMS.index(a.form)
            nb = float(max(t * b * G, 1))
            lab, tb, off, cnt = packed.labels.data_ptr(), packed.boxes.data_ptr(), packed.offsets.data_ptr(), packed.counts_c
            fns = [
                ("match_cost", lambda: lib.lwdetr_match_cost(arr, nl, b, nq, ncls, lab, tb, off, cnt, 2.0, 5.0, 2.0, 0.25, ws.cost.data_ptr(), dt, st)),
                ("match_assign_groups", lambda: lib.lwdetr_match_assign_groups(ws.cost.data_ptr(), off, cnt, nl, b, nq, G, ws.idx_q.data_ptr(),
                                                                               ws.idx_t.data_ptr(), ws.status.data_ptr(), ws.steps.data_ptr(), st)),
                ("train_partials", lambda: lib.lwdetr_criterion_train_partials(arr, nl, b, nq, ncls, lab, tb, off, cnt, ws.idx_q.data_ptr(),
                                                                               ws.idx_t.data_ptr(), G, form, 0.25, ws.partials.data_ptr(), dt, st)),
                ("train_finish", lambda: lib.lwdetr_criterion_train_finish(ws.partials.data_ptr(), arr, off, cnt, nl, b, nq, G, form, nb, out.data_ptr(), st)),
                ("backward", lambda: lib.lwdetr_criterion_backward(arr, garr, nl, b, nq, ncls, lab, tb, off, cnt, ws.idx_q.data_ptr(), ws.idx_t.data_ptr(),
                                                                   G, form, 0.25, nb, up.data_ptr(), dt, st)),
            ]
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(fns) + 1)] for _ in range(a.n)]
            for r in range(a.n + 5):
                e = ev[max(r - 5, 0)]
                e[0].record()
                for k, (_, fn) in enumerate(fns):
                    assert fn() == 0
                    e[k + 1].record()
            torch.cuda.synchronize(dev)
            ms = [stats([e[k].elapsed_time(e[k + 1]) for e in ev])[0] for k in range(len(fns))]
            print("phases by HIP events (median ms): " + ", ".join(f"{n} {v:.3f}" for (n, _), v in zip(fns, ms)) +
                  f"; largest: {fns[max(range(len(ms)), key=ms.__getitem__)][0]}")
            steps = m.steps().flatten().tolist()
            print(f"solver steps per problem: min {min(steps)} median {sorted(steps)[len(steps) // 2]} max {max(steps)} (bounds {t} .. {t * (t + 1) // 2}); "
                  f"status non-zero: {int(m.status().ne(0).sum())}")

            # the evaluation criterion on one group's queries: the floor of the shared part
            one = [(lg[:, :gw].contiguous(), bx[:, :gw].contiguous()) for lg, bx in plain]
            old = M.SetCriterion(ncls, M.HungarianMatcher(focal_alpha=0.25, **R.COST_W), {}, 0.25, ["labels", "boxes", "cardinality"],
                                 ia_bce_loss=a.form == "iabce")
            r = timed(lambda: old(R.as_outputs(one), targets))
            print(f"{'eval criterion, one group of ' + str(gw):36s} median {r[0]:9.3f} ms   min {r[1]:9.3f}   max {r[2]:9.3f}")


if __name__ == "__main__":
    main()
