"""The tail of a training step on the library's multi-tensor kernels (csrc/optim.hip): gradient-norm clip, AdamW over one parameter group
per parameter, and the model EMA - what the reference runs as ``clip_grad_norm_`` + ``torch.optim.AdamW.step`` + ``ModelEma.update``
(engine.py:76-83, util/get_param_dicts.py, util/utils.py:7-32), several thousand launches over a few hundred bytes each.

    param_dicts = get_param_dict(args, model)
    ema_m = ModelEma(model, decay=args.ema_decay)
    optimizer = NativeAdamW(param_dicts, lr=args.lr, weight_decay=args.weight_decay, max_norm=args.clip_max_norm, ema=ema_m)
    ...
    losses.backward(); optimizer.step(); ema_m.update(model)        # three launches; update() finds its work done

``NativeAdamW`` keeps torch's ``param_groups`` / ``state`` / ``state_dict()``; only ``step()`` is replaced. ``clip_grad_norm_`` and a
``ModelEma`` that is not attached to an optimizer are the stand-alone forms of the same kernels.

Differences from the reference sequence, both deliberate: the fused step does not write the clipped gradient back to ``p.grad`` (it is scaled in
registers), and the total norm is an f64 sum of per-chunk f32 sums of squares, not a norm of per-tensor norms.

Tensors in host memory go through the library's host form of the same per-element functions (``NativeAdamW(..., host=True)``, a ``ModelEma`` of
a CPU model): that is how the tests run this layer without a GPU. There is no eager-PyTorch path.
"""
import copy
import ctypes as C

import numpy as np
import torch

from . import _native as N

__all__ = ["get_param_dict", "get_vit_lr_decay_rate", "get_vit_weight_decay_rate", "NativeAdamW", "ModelEma", "clip_grad_norm_", "drop_scheduler", "CHUNK"]

CHUNK = N.MT_CHUNK
_TENSOR_DT = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("ema", "<u8"), ("numel", "<i8"), ("kind", "<i4"), ("skip", "<i4"),
                       ("decay_mul", "<f4"), ("neg_step_size", "<f4"), ("bc2_sqrt", "<f4"), ("reserved", "<i4")])
_CHUNK_DT = np.dtype([("tensor", "<i4"), ("count", "<i4"), ("offset", "<i8")])
assert _TENSOR_DT.itemsize == C.sizeof(N.MtTensor) and _CHUNK_DT.itemsize == C.sizeof(N.MtChunk)
_RING = 4


# ------------------------------------------------------------------------------------------------ drop-rate schedule
def drop_scheduler(drop_rate, epochs, niter_per_ep, cutoff_epoch=0, mode="standard", schedule="constant"):
    """The per-iteration drop-path (or dropout) rate as a numpy array of epochs * niter_per_ep entries (util/drop_scheduler.py): ``standard`` holds
    ``drop_rate`` throughout; ``early`` holds it (``constant``) or runs it down to 0 (``linear``) over the first ``cutoff_epoch`` epochs and is 0
    afterwards; ``late`` is 0 for ``cutoff_epoch`` epochs and ``drop_rate`` afterwards. ``model.update_drop_path(schedule[it], depth)`` per step."""
    assert mode in ("standard", "early", "late")
    total = epochs * niter_per_ep
    if mode == "standard":
        return np.full(total, drop_rate)
    head, tail = cutoff_epoch * niter_per_ep, (epochs - cutoff_epoch) * niter_per_ep
    if mode == "early":
        assert schedule in ("constant", "linear")
        first = np.full(head, drop_rate) if schedule == "constant" else np.linspace(drop_rate, 0, head)
        out = np.concatenate((first, np.full(tail, 0)))
    else:
        assert schedule in ("constant",)
        out = np.concatenate((np.full(head, 0), np.full(tail, drop_rate)))
    assert len(out) == total
    return out


# ------------------------------------------------------------------------------------------------ parameter groups
def get_vit_lr_decay_rate(name, lr_decay_rate=1.0, num_layers=12):
    """Layer-wise lr decay of the ViT (util/get_param_dicts.py:13-31): pos_embed / patch_embed are layer 0, block i is layer i + 1."""
    layer_id = num_layers + 1
    if name.startswith("backbone"):
        if ".pos_embed" in name or ".patch_embed" in name:
            layer_id = 0
        elif ".blocks." in name and ".residual." not in name:
            layer_id = int(name[name.find(".blocks."):].split(".")[2]) + 1
    return lr_decay_rate ** (num_layers + 1 - layer_id)


def get_vit_weight_decay_rate(name, weight_decay_rate=1.0):
    """No weight decay on gamma / pos_embed / rel_pos / bias / norm parameters (util/get_param_dicts.py:34-38)."""
    if ("gamma" in name) or ("pos_embed" in name) or ("rel_pos" in name) or ("bias" in name) or ("norm" in name):
        return 0.0
    return weight_decay_rate


def get_param_dict(args, model):
    """One parameter group per parameter, in the reference's order (util/get_param_dicts.py:41-72, models/backbone/backbone.py:173-189):
    every other parameter at ``lr``, then the ViT encoder at ``lr_encoder`` x layer decay x ``lr_component_decay``^2 with its own
    ``weight_decay``, then the decoder at ``lr * lr_component_decay``. Groups without a ``weight_decay`` key take the optimizer's."""
    backbone = model.backbone[0]
    if "vit" not in backbone.name:
        raise NotImplementedError(f"get_param_dict: backbone {backbone.name!r} (this package builds the ViT encoders only)")
    backbone_pairs = {}
    for n, p in backbone.named_parameters():
        n = "backbone.0." + n
        if "backbone.0.encoder" in n and p.requires_grad:
            lr = args.lr_encoder * get_vit_lr_decay_rate(n, lr_decay_rate=args.lr_vit_layer_decay,
                                                         num_layers=args.vit_encoder_num_layers) * args.lr_component_decay ** 2
            backbone_pairs[n] = {"params": p, "lr": lr, "weight_decay": args.weight_decay * get_vit_weight_decay_rate(n)}
    decoder_key = "transformer.decoder"
    named = list(model.named_parameters())
    decoder = [{"params": p, "lr": args.lr * args.lr_component_decay} for n, p in named if decoder_key in n and p.requires_grad]
    other = [{"params": p, "lr": args.lr} for n, p in named if n not in backbone_pairs and decoder_key not in n and p.requires_grad]
    return other + list(backbone_pairs.values()) + decoder


# ------------------------------------------------------------------------------------------------ tables
def _chunks_for(numels: np.ndarray) -> np.ndarray:
    per = (numels + CHUNK - 1) // CHUNK
    first = np.cumsum(per) - per
    out = np.zeros(int(per.sum()), dtype=_CHUNK_DT)
    tensor = np.repeat(np.arange(len(numels), dtype=np.int64), per)
    offset = (np.arange(len(out), dtype=np.int64) - first[tensor]) * CHUNK
    out["tensor"], out["offset"], out["count"] = tensor, offset, np.minimum(numels[tensor] - offset, CHUNK)
    return out


class _Tables:
    """A tensor table and its chunk table. On a GPU: the chunk table is uploaded once; the tensor table goes up through a ring of pinned
    buffers, one asynchronous copy per refresh - a pinned buffer is rewritten only after the event behind its last copy (``_RING`` refreshes
    ago) has passed, so the host never waits for the queue unless it is that many steps ahead. In host memory the arrays are the tables."""

    def __init__(self, numels, kinds, device):
        self.device = torch.device(device)
        self.host = self.device.type != "cuda"
        self.rec = np.zeros(len(numels), dtype=_TENSOR_DT)
        self.rec["numel"], self.rec["kind"] = numels, kinds
        self.rec["decay_mul"], self.rec["bc2_sqrt"] = 1.0, 1.0
        self.chunks = _chunks_for(self.rec["numel"])
        self.n, self.nchunks = len(self.rec), len(self.chunks)
        self.uploaded = None
        # the chunk table is fixed from here on; later refreshes change pointers and scalars only
        N.check(N.lib().lwdetr_mt_check(self.rec.ctypes.data, self.n, self.chunks.ctypes.data, self.nchunks), "lwdetr_mt_check")
        if self.host:
            self.norm_clip = torch.zeros(4, dtype=torch.float32)
            return
        self.norm_clip = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.partials = torch.empty(self.nchunks, dtype=torch.float32, device=self.device)
        self.dev_chunks = torch.from_numpy(self.chunks.view(np.uint8).copy()).to(self.device)
        self.dev_rec = torch.empty(self.rec.nbytes, dtype=torch.uint8, device=self.device)
        self.pinned = [torch.empty(self.rec.nbytes, dtype=torch.uint8).pin_memory() for _ in range(_RING)]
        self.views = [t.numpy().view(_TENSOR_DT) for t in self.pinned]
        self.events = [None] * _RING
        self.slot = 0

    def upload(self, force=True):
        """Make the kernels see ``self.rec``. ``force=False`` skips the copy when the records are what was uploaded last."""
        if self.host:
            return
        if not force and self.uploaded is not None and self.uploaded.tobytes() == self.rec.tobytes():
            return
        i = self.slot
        self.slot = (i + 1) % _RING
        if self.events[i] is not None:
            self.events[i].synchronize()
        self.views[i][:] = self.rec
        with torch.cuda.device(self.device):
            self.dev_rec.copy_(self.pinned[i], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self.events[i] = ev
        self.uploaded = None if force else self.rec.copy()

    def norm(self, max_norm):
        l = N.lib()
        if self.host:
            N.check(l.lwdetr_mt_norm_host(self.rec.ctypes.data, self.n, self.chunks.ctypes.data, self.nchunks, float(max_norm),
                                          self.norm_clip.data_ptr()), "lwdetr_mt_norm_host")
            return
        st = N.stream_ptr(self.device)
        N.check(l.lwdetr_mt_sumsq(self.dev_rec.data_ptr(), self.n, self.dev_chunks.data_ptr(), self.nchunks, self.partials.data_ptr(), st),
                "lwdetr_mt_sumsq")
        N.check(l.lwdetr_mt_norm_finish(self.partials.data_ptr(), self.nchunks, float(max_norm), self.norm_clip.data_ptr(), st),
                "lwdetr_mt_norm_finish")

    def step(self, hyper, flags, clipped):
        l = N.lib()
        nc = self.norm_clip.data_ptr() if clipped else None
        hp = C.byref(hyper) if hyper is not None else None
        if self.host:
            N.check(l.lwdetr_mt_step_host(self.rec.ctypes.data, self.n, self.chunks.ctypes.data, self.nchunks, hp, flags, nc), "lwdetr_mt_step_host")
            return
        N.check(l.lwdetr_mt_step(self.dev_rec.data_ptr(), self.n, self.dev_chunks.data_ptr(), self.nchunks, hp, flags, nc,
                                 N.stream_ptr(self.device)), "lwdetr_mt_step")


def _hyper(beta1=0.0, beta2=0.0, eps=0.0, decay=None):
    h = N.MtHyper()
    h.one_minus_beta1, h.beta2, h.one_minus_beta2, h.eps = 1 - beta1, beta2, 1 - beta2, eps       # doubles, rounded once by the assignment
    if decay is not None:
        h.ema_decay, h.ema_one_minus_decay = decay, 1. - decay
    return h


def _ptrs(tensors):
    return np.fromiter((0 if t is None else t.data_ptr() for t in tensors), dtype=np.uint64, count=len(tensors))


# ------------------------------------------------------------------------------------------------ EMA
class ModelEma(torch.nn.Module):
    """The reference's ``ModelEma`` (util/utils.py:7-32): ``.module`` is a deep copy of the model in eval mode, ``update(model)`` moves every
    state-dict entry by ``decay * e + (1 - decay) * m`` (f32; an int64 buffer such as ``num_batches_tracked`` gets the truncated f32 result, as
    the reference's ``copy_`` gives), ``set(model)`` copies. One launch each. Passed to ``NativeAdamW(ema=...)`` it is bound to the model it was
    built from: the optimizer's launch updates the EMA from registers and the ``update(model)`` that follows that step returns at once."""

    def __init__(self, model, decay=0.9997, device=None):
        super().__init__()
        if device is not None:
            raise ValueError("lwdetr_amd.train.ModelEma keeps the EMA on the model's device (device=None)")
        self.module = copy.deepcopy(model)
        self.module.eval()
        self.decay = decay
        self.device = None
        self._source = (model,)            # a tuple: not registered as a submodule
        self._tables = None
        self._entries = None
        self._covered = False

    @staticmethod
    def _kind(x, e):
        if x.dtype != e.dtype or x.shape != e.shape or x.device != e.device or not (x.is_contiguous() and e.is_contiguous()):
            raise ValueError("ModelEma: a state-dict entry and its EMA copy differ in dtype, shape, device or are not contiguous")
        if x.dtype == torch.float32:
            return N.MT_EMA_F32
        if x.dtype == torch.int64:
            return N.MT_EMA_I64
        raise ValueError(f"ModelEma: state-dict entries of dtype {x.dtype} are not supported (float32 and int64 are)")

    def entries(self, model):
        """[(model tensor, EMA tensor, kind)] over the non-empty state-dict entries, in state-dict order; cached while the identities of the
        entries hold on both sides. The tensors are the modules' own objects: pointers are read from them at every call, so a ``.data``
        that was swapped is followed, and an entry that was replaced rebuilds the list."""
        src = list(model.state_dict(keep_vars=True).values())
        dst = list(self.module.state_dict(keep_vars=True).values())
        cur = self._entries
        if cur is not None and len(cur[0]) == len(src) and len(cur[2]) == len(dst) and all(a is b for a, b in zip(cur[0], src)) and \
                all(a is b for a, b in zip(cur[2], dst)):
            return cur[1]
        if len(src) != len(dst):
            raise ValueError("ModelEma: the model's state dict does not match the EMA copy's")
        ent = [(x, e, self._kind(x, e)) for x, e in zip(src, dst) if x.numel() > 0]
        if len({e.data_ptr() for _, e, _ in ent}) != len(ent):
            raise ValueError("ModelEma: tied state-dict entries are not supported")
        devs = {x.device for x, _, _ in ent}
        if len(devs) != 1:
            raise ValueError("ModelEma: the model must live on one device")
        self._entries = (src, ent, dst)
        self._tables = None
        return ent

    def _run(self, model, flags):
        ent = self.entries(model)
        tb = self._tables
        if tb is None:
            tb = self._tables = _Tables(np.array([x.numel() for x, _, _ in ent], dtype=np.int64), [k for _, _, k in ent], ent[0][0].device)
        tb.rec["p"], tb.rec["ema"] = _ptrs([x for x, _, _ in ent]), _ptrs([e for _, e, _ in ent])
        tb.upload(force=False)
        with torch.no_grad():
            tb.step(_hyper(decay=self.decay), flags, clipped=False)

    def update(self, model):
        if self._covered and model is self._source[0]:
            self._covered = False
            return
        self._run(model, N.MT_EMA)

    def set(self, model):
        self._run(model, N.MT_EMA_SET)


# ------------------------------------------------------------------------------------------------ optimizer
class NativeAdamW(torch.optim.AdamW):
    """``torch.optim.AdamW`` whose ``step()`` is at most three launches for any number of parameter groups: sum of squares of the gradients and
    the norm / clip coefficient (only with ``max_norm > 0``), then one pass that scales the gradient in registers, applies AdamW with every
    tensor's own ``lr`` / ``weight_decay`` / step count and, with ``ema=``, updates the EMA copy from the new value.

    ``param_groups``, ``state`` (``step`` a CPU f32 tensor, ``exp_avg``, ``exp_avg_sq``), ``state_dict()`` and ``load_state_dict()`` are
    torch's: a checkpoint written by ``torch.optim.AdamW`` loads and one written here loads there; schedulers work. ``step()`` rereads every
    group's ``lr`` and ``weight_decay``. A parameter whose ``grad`` is None keeps its state and step count (its EMA entry still moves).
    ``last_total_norm`` is a 0-dim tensor on the parameters' device, rewritten by every clipped step. The clipped gradient is not written
    back to ``p.grad``."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False, foreach=None,
                 capturable=False, differentiable=False, fused=None, max_norm=0.0, ema=None, host=False):
        for name, val in (("amsgrad", amsgrad), ("maximize", maximize), ("capturable", capturable), ("differentiable", differentiable)):
            if val:
                raise ValueError(f"NativeAdamW: {name}=True is not supported")
        if isinstance(lr, torch.Tensor):
            raise ValueError("NativeAdamW: a tensor lr is not supported")
        if max_norm is None or not (float(max_norm) >= 0.0):
            raise ValueError(f"NativeAdamW: max_norm must be >= 0 (0 = no clipping), got {max_norm}")
        if ema is not None and not isinstance(ema, ModelEma):
            raise ValueError("NativeAdamW: ema must be a lwdetr_amd.train.ModelEma")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.max_norm = float(max_norm)
        self.ema = ema
        self.host = bool(host)
        self._tables = None
        self._sig = None
        self._check_params()
        dev = self._params()[0].device
        self.last_total_norm = torch.zeros((), dtype=torch.float32, device=dev)

    def _params(self):
        return [p for g in self.param_groups for p in g["params"]]

    def _check_params(self):
        ps = self._params()
        dev = ps[0].device
        for p in ps:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.is_sparse or p.device != dev or p.numel() == 0:
                raise ValueError("NativeAdamW: every parameter must be a non-empty contiguous float32 tensor on one device")
        if self.host != (dev.type != "cuda"):
            raise ValueError("NativeAdamW: the parameters must live on one GPU" if not self.host else
                             "NativeAdamW(host=True) is the host form: the parameters must live in host memory")
        g0 = self.param_groups[0]
        for g in self.param_groups:
            if isinstance(g["lr"], torch.Tensor) or tuple(g["betas"]) != tuple(g0["betas"]) or g["eps"] != g0["eps"]:
                raise ValueError("NativeAdamW: betas and eps must be the same in every group, and lr a float")
            if g["amsgrad"] or g["maximize"] or g["capturable"] or g["differentiable"]:
                raise ValueError("NativeAdamW: amsgrad / maximize / capturable / differentiable groups are not supported")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if hasattr(self, "host"):
            self._check_params()
            self._tables = None

    def _build(self, ps):
        """The table: the parameters in group order, then - with an EMA - the state-dict entries that are not optimizer parameters."""
        extra, ema_of = [], {}
        if self.ema is not None:
            index = {(p.data_ptr(), p.numel()): i for i, p in enumerate(ps)}
            for x, e, kind in self.ema.entries(self.ema._source[0]):
                i = index.get((x.data_ptr(), x.numel())) if kind == N.MT_EMA_F32 else None
                if i is None:
                    extra.append((x, e, kind))
                else:
                    ema_of[i] = e
            if extra and extra[0][0].device != ps[0].device:
                raise ValueError("NativeAdamW: the EMA's model lives on another device than the parameters")
        n = len(ps)
        tb = _Tables(np.array([p.numel() for p in ps] + [x.numel() for x, _, _ in extra], dtype=np.int64),
                     [N.MT_PARAM] * n + [k for _, _, k in extra], ps[0].device)
        tb.ema_tensors = [ema_of.get(i) for i in range(n)] + [e for _, e, _ in extra]
        tb.extra = [x for x, _, _ in extra]
        tb.ema_entries = self.ema._entries[1] if self.ema is not None else None
        return tb

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        ps = self._params()
        n = len(ps)
        g0 = self.param_groups[0]
        beta1, beta2 = g0["betas"]
        lr, wd = np.empty(n), np.empty(n)
        i = 0
        for g in self.param_groups:
            k = len(g["params"])
            if isinstance(g["lr"], torch.Tensor) or tuple(g["betas"]) != (beta1, beta2) or g["eps"] != g0["eps"]:
                raise ValueError("NativeAdamW: betas and eps must be the same in every group, and lr a float")
            lr[i:i + k], wd[i:i + k] = g["lr"], g["weight_decay"]
            i += k
        sig = tuple(map(id, ps))
        tb = self._tables
        if tb is None or sig != self._sig or (self.ema is not None and self.ema.entries(self.ema._source[0]) is not tb.ema_entries):
            tb = self._tables = self._build(ps)
            self._sig = sig
        dev = ps[0].device
        grads, steps, active, ms, vs = [], [], [], [], []
        zero = torch.tensor(0.0, dtype=torch.float32)
        for p in ps:
            gr = p.grad
            if gr is not None:
                st = self.state[p]
                if gr.is_sparse:
                    raise ValueError("NativeAdamW: sparse gradients are not supported")
                if gr.dtype != torch.float32 or gr.device != dev or not gr.is_contiguous():
                    raise ValueError("NativeAdamW: every gradient must be a contiguous float32 tensor on the parameters' device")
                if len(st) == 0:                     # state appears with the first gradient, as in torch
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                for a in (m, v):
                    if a.shape != p.shape or a.dtype != torch.float32 or a.device != dev or not a.is_contiguous():
                        raise ValueError("NativeAdamW: exp_avg / exp_avg_sq must be contiguous float32 tensors of the parameter's shape and device")
                if st["step"].device.type != "cpu":
                    raise ValueError("NativeAdamW: state['step'] must be a CPU tensor (torch's default for a non-capturable optimizer)")
                active.append(st["step"])
                steps.append(st["step"])
                ms.append(m)
                vs.append(v)
            else:                                    # no gradient: state and step count stay as they are, the record is skipped
                steps.append(zero)
                ms.append(None)
                vs.append(None)
            grads.append(gr)
        if active:
            torch._foreach_add_(active, 1.0)
        try:
            t = torch.stack(steps)
        except RuntimeError:                         # a loaded checkpoint may carry steps of another shape or dtype
            t = torch.stack([x.reshape(()).float() for x in steps])
        t = t.double().numpy()
        rec = tb.rec
        if any(p.numel() != m for p, m in zip(ps, rec["numel"][:n].tolist())):
            raise ValueError("NativeAdamW: a parameter changed its size")
        rec["p"][:n], rec["g"][:n], rec["m"][:n], rec["v"][:n] = _ptrs(ps), _ptrs(grads), _ptrs(ms), _ptrs(vs)
        rec["p"][n:] = _ptrs(tb.extra)
        rec["ema"] = _ptrs(tb.ema_tensors)
        rec["skip"][:n] = [gr is None for gr in grads]
        with np.errstate(divide="ignore", invalid="ignore"):          # a parameter that never had a gradient is at step 0: its scalars are not used
            rec["decay_mul"][:n] = 1 - lr * wd
            rec["neg_step_size"][:n] = -(lr / (1 - beta1 ** t))
            rec["bc2_sqrt"][:n] = (1 - beta2 ** t) ** 0.5
        tb.upload()
        clipped = self.max_norm > 0.0
        if clipped:
            tb.norm(self.max_norm)
        flags = N.MT_ADAMW | (N.MT_EMA if self.ema is not None else 0)
        tb.step(_hyper(beta1, beta2, g0["eps"], self.ema.decay if self.ema is not None else None), flags, clipped)
        self.last_total_norm = tb.norm_clip[0]
        if self.ema is not None:
            self.ema._covered = True
        return loss


# ------------------------------------------------------------------------------------------------ stand-alone clip
_clip_tables = {}


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """``torch.nn.utils.clip_grad_norm_`` for the 2-norm in three launches: the gradients are multiplied by
    ``min(1, max_norm / (total_norm + 1e-6))`` in place (also when that is 1, as torch does). Returns the total norm as a 0-dim tensor on
    the gradients' device, without waiting for it."""
    if float(norm_type) != 2.0:
        raise ValueError("lwdetr_amd.train.clip_grad_norm_ computes the 2-norm only")
    if not (float(max_norm) > 0.0):
        raise ValueError(f"clip_grad_norm_: max_norm must be > 0, got {max_norm}")
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        return torch.tensor(0.0)
    dev = grads[0].device
    for g in grads:
        if g.is_sparse or g.dtype != torch.float32 or g.device != dev or not g.is_contiguous():
            raise ValueError("clip_grad_norm_: every gradient must be a contiguous dense float32 tensor on one device")
    grads = [g for g in grads if g.numel() > 0]
    key = (dev, tuple(g.numel() for g in grads))
    tb = _clip_tables.get(key)
    if tb is None:
        _clip_tables.clear()                                     # one training loop has one gradient set
        tb = _clip_tables[key] = _Tables(np.array(key[1], dtype=np.int64), N.MT_PARAM, dev)
    tb.rec["g"] = _ptrs(grads)
    tb.upload()
    with torch.no_grad():
        tb.norm(max_norm)
        tb.step(None, N.MT_SCALE_GRADS, clipped=True)
        return tb.norm_clip[0].clone()
