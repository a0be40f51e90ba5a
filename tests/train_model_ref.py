"""What the training-model tests and tools/gen_golden_train_model.py share: the two reduced configurations, their inputs, the loss, the
recorded quantities and the figures.

The golden (tests/golden/train_model.npz) is recorded from the unmodified reference model in train mode on the CPU, in float64 and in float32.
Weights are ``synth_state_dict(seed)``, images ``synth_images(seed=IMAGE_SEED)``; the loss is sum(output * cotangent) over every tensor of the
output dict with the cotangents below. Recorded per configuration: every output (float64), the two-stage indices, the L2 norm and the sum of
every parameter's float64 gradient, the float64 gradient itself of the tensors in ``full_grad_keys`` (a tensor above SAMPLE_CAP elements as the
strided sample ``sample_idx``), the BatchNorm buffers after the step, and for every one of these the figure of the reference's own float32 run
against its float64 run.

Figures: ``two_stage_ref.figure`` = max |a - b| / max |b| of every recorded quantity. The gradient norms of all parameters are ONE quantity (a
vector with one entry per parameter), and so are the sums: several parameters have a gradient that is zero in exact arithmetic (the key bias of
a softmax attention, for one), whose computed norm is rounding noise and has no scale of its own. The yardstick of a group (outputs, full gradients, gradient norms and sums, BatchNorm statistics) is the largest recorded float32
figure within the group, times MARGIN.
"""
import os

import numpy as np
import torch

import two_stage_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_PATH = os.path.join(ROOT, "tests", "golden", "train_model.npz")
MARGIN = R.MARGIN
F64_TOL = 1e-12            # the sibling host tests' float64 bound (tests/test_msda_train_host.py: 1e-12 of the magnitude)
IMAGE_SEED = 4321
COTANGENT_SEED = 99
SAMPLE_CAP = 8192
REDUCED = dict(vit_encoder_num_layers=4, window_block_indexes=[0, 2], out_feature_indexes=[1, 3], num_queries=10, group_detr=3, dec_layers=2)
RECORDINGS = {"tiny": ("tiny", [(128, 128), (96, 128)]), "large": ("large", [(128, 128), (128, 64)])}
GROUPS = ("out", "gfull", "gnorm", "bn")


def args_of(name):
    import lwdetr_amd
    return lwdetr_amd.get_args(RECORDINGS[name][0], **{k: (list(v) if isinstance(v, list) else v) for k, v in REDUCED.items()})


def images_of(name):
    """The recording's images as a list of (3, h, w) float32 tensors: the second is smaller, so the batch is padded."""
    from lwdetr_amd.synth import synth_images
    dims = RECORDINGS[name][1]
    hmax, wmax = max(d[0] for d in dims), max(d[1] for d in dims)
    full = synth_images(len(dims), hmax, wmax, seed=IMAGE_SEED)
    return [full[i, :, :h, :w].clone() for i, (h, w) in enumerate(dims)]


def flat_outputs(out):
    """The output dict as {name: tensor} in one fixed order."""
    flat = {"pred_logits": out["pred_logits"], "pred_boxes": out["pred_boxes"]}
    for j, aux in enumerate(out.get("aux_outputs", [])):
        flat[f"aux{j}_logits"], flat[f"aux{j}_boxes"] = aux["pred_logits"], aux["pred_boxes"]
    flat["enc_logits"], flat["enc_boxes"] = out["enc_outputs"]["pred_logits"], out["enc_outputs"]["pred_boxes"]
    return flat


def cotangents(flat):
    g = torch.Generator().manual_seed(COTANGENT_SEED)
    return {k: torch.randn(v.shape, generator=g, dtype=torch.float64) for k, v in flat.items()}


def loss_of(flat):
    ct = cotangents(flat)
    return sum((v * ct[k].to(device=v.device, dtype=v.dtype)).sum() for k, v in flat.items())


def full_grad_keys(keys):
    """The parameters whose whole gradient is recorded: all norms of ViT block 1 and decoder layer 0, gamma_1 / gamma_2 and q_bias of block 1,
    refpoint_embed, pos_embed, the first stage's LayerNorm2d and its cv1 BatchNorm."""
    want = []
    for k in keys:
        if k.startswith("backbone.0.encoder.blocks.1.") and (".norm" in k or k.endswith(("gamma_1", "gamma_2", "q_bias"))):
            want.append(k)
        elif k.startswith("transformer.decoder.layers.0.norm") or k.startswith("transformer.decoder.norm."):
            want.append(k)
        elif k in ("refpoint_embed.weight", "backbone.0.encoder.pos_embed"):
            want.append(k)
        elif k.startswith("backbone.0.projector.stages.0.1.") or k.startswith("backbone.0.projector.stages.0.0.cv1.bn.") and k.endswith(("weight", "bias")):
            want.append(k)
    return want


def sample_idx(n):
    if n <= SAMPLE_CAP:
        return np.arange(n)
    stride = -(-n // SAMPLE_CAP)
    stride += 1 - (stride % 2)
    return np.arange(0, n, stride)[:SAMPLE_CAP]


def sampled(t):
    flat = t.detach().reshape(-1)
    return flat[torch.from_numpy(sample_idx(flat.numel())).to(flat.device)]


def quantities(model, out, idx):
    """Runs the backward of the loss and returns every recorded quantity as {key: CPU tensor}: out.*, idx, gnorm / gsum (vectors over the named
    parameters), gfull.*, bn.* (the float BatchNorm buffers)."""
    flat = flat_outputs(out)
    model.zero_grad(set_to_none=True)
    loss_of(flat).backward()
    q = {f"out.{k}": v.detach().cpu() for k, v in flat.items()}
    q["idx"] = idx.detach().cpu()
    names = [n for n, _ in model.named_parameters()]
    grads = {n: (p.grad if p.grad is not None else torch.zeros_like(p)).detach() for n, p in model.named_parameters()}
    q["gnorm"] = torch.stack([grads[n].double().norm() for n in names]).cpu()
    q["gsum"] = torch.stack([grads[n].double().sum() for n in names]).cpu()
    for k in full_grad_keys(names):
        q[f"gfull.{k}"] = sampled(grads[k]).cpu()
    for k, v in model.state_dict().items():
        if k.endswith(("running_mean", "running_var")):
            q[f"bn.{k}"] = v.detach().cpu().clone()
    return q, names


def figures(q, ref):
    """{quantity key: figure of q against ref} for every key that carries one (see the module docstring)."""
    fig = {}
    for k in ref:
        if k.startswith(("out.", "gfull.", "bn.")):
            fig[k] = R.figure(q[k], ref[k])
    fig["gnorm"], fig["gsum"] = R.figure(q["gnorm"], ref["gnorm"]), R.figure(q["gsum"], ref["gsum"])
    return fig


def group_of(key):
    return "gnorm" if key in ("gnorm", "gsum") else key.split(".", 1)[0]


def group_figures(fig):
    out = {g: 0.0 for g in GROUPS}
    for k, v in fig.items():
        out[group_of(k)] = max(out[group_of(k)], v)
    return out


def load_golden(name):
    """-> (reference quantities {key: tensor}, recorded float32 figures {key: float}, parameter names, seed) of one recording."""
    z = np.load(GOLDEN_PATH, allow_pickle=False)
    pre = name + "__"
    ref = {k[len(pre) + 3:]: torch.from_numpy(np.asarray(z[k])) for k in z.files if k.startswith(pre + "q__")}
    fig = {k[len(pre) + 3:]: float(z[k]) for k in z.files if k.startswith(pre + "f__")}
    names = [str(s) for s in z[pre + "param_names"]]
    return ref, fig, names, int(z[pre + "seed"])


def build_native(name, seed, dtype=torch.float32, device="cpu"):
    """This package's model for a recording, loaded with the recording's weights, in train mode."""
    import lwdetr_amd
    from lwdetr_amd.synth import synth_state_dict
    model, _, _ = lwdetr_amd.build_model(args_of(name))
    model.load_state_dict(synth_state_dict(model.state_dict(), seed=seed), strict=True)
    return model.to(device=device, dtype=dtype).train()


def run_native(model, name, fused, device="cpu", dtype=torch.float32):
    from lwdetr_amd.models.train_forward import differentiable_forward
    imgs = [t.to(device=device, dtype=dtype) for t in images_of(name)]
    col = {}
    out = differentiable_forward(model, imgs, fused=fused, collect=col)
    return out, col["topk_idx"]


def is_finite(q):
    return all(bool(torch.isfinite(v.double()).all()) for v in q.values())

