"""Helpers of the two-stage selection tests: the launch-form record of csrc/two_stage_train.hip, a stand-in for the reference's Transformer
(its attribute names and state-dict keys, no reference code) and the reference's loop written in torch."""
import contextlib

import torch
import torch.nn as nn
import torch.nn.functional as F


@contextlib.contextmanager
def two_stage_served_by(forms):
    """The lwdetr_two_stage_* launches inside the block went to exactly the instantiations `forms` ({name: launches}), and to no other."""
    from lwdetr_amd import _native
    before = _native.two_stage_path_counts()
    for f in forms:
        assert f in before, f"unknown two-stage kernel form {f!r}: {sorted(before)}"
    yield
    torch.cuda.synchronize()
    after = _native.two_stage_path_counts()
    delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
    assert delta == dict(forms), f"launch forms {delta}, expected {dict(forms)}"


class BoxHead(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.num_layers = 3
        self.layers = nn.ModuleList([nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, 4)])

    def forward(self, x):
        for i, layer in enumerate(self.layers):
            x = F.relu(layer(x)) if i < 2 else layer(x)
        return x


class Recorder(nn.Module):
    def __init__(self):
        super().__init__()
        self.seen = None

    def forward(self, tgt, memory, **kw):
        self.seen = dict(tgt=tgt, memory=memory, **kw)
        return tgt.unsqueeze(0), kw["refpoints_unsigmoid"].unsqueeze(0)


class StandInTransformer(nn.Module):
    """The attributes ``patch_two_stage`` looks for, under the reference's names; ``forward`` is a marker that the patch must replace."""

    def __init__(self, d, groups, num_queries, ncls, bbox_reparam=True, two_stage=True):
        super().__init__()
        self.decoder = Recorder()
        self.two_stage, self.group_detr, self.num_queries, self.bbox_reparam, self.d_model = two_stage, groups, num_queries, bbox_reparam, d
        self.enc_output = nn.ModuleList([nn.Linear(d, d) for _ in range(groups)])
        self.enc_output_norm = nn.ModuleList([nn.LayerNorm(d) for _ in range(groups)])
        self.enc_out_class_embed = nn.ModuleList([nn.Linear(d, ncls) for _ in range(groups)])
        self.enc_out_bbox_embed = nn.ModuleList([BoxHead(d) for _ in range(groups)])

    def forward(self, *a, **k):
        return "unpatched"


def load_case(module, inp):
    """Copies a two_stage_ref case's stacked weights into a StandInTransformer's own parameters."""
    with torch.no_grad():
        for g in range(module.group_detr):
            module.enc_output[g].weight.copy_(inp["W_eo"][g]); module.enc_output[g].bias.copy_(inp["b_eo"][g])
            module.enc_output_norm[g].weight.copy_(inp["ln_w"][g]); module.enc_output_norm[g].bias.copy_(inp["ln_b"][g])
            module.enc_out_class_embed[g].weight.copy_(inp["W_cls"][g]); module.enc_out_class_embed[g].bias.copy_(inp["b_cls"][g])
            for i in range(3):
                module.enc_out_bbox_embed[g].layers[i].weight.copy_(inp["W_box"][i][g])
                module.enc_out_bbox_embed[g].layers[i].bias.copy_(inp["b_box"][i][g])
    return module


def reference_loop(memory, valid, props, module, num_queries, groups, bbox_reparam):
    """The reference's per-group loop over ALL rows (transformer.py:230-264) in torch, under autograd: what the operator is measured against."""
    x = memory * valid.unsqueeze(-1).to(memory.dtype)
    props = props.to(memory.dtype)
    d = memory.shape[-1]
    mts, bts = [], []
    for g in range(groups):
        y = module.enc_output_norm[g](module.enc_output[g](x))
        cls = module.enc_out_class_embed[g](y)
        delta = module.enc_out_bbox_embed[g](y)
        if bbox_reparam:
            coord = torch.cat([delta[..., :2] * props[..., 2:] + props[..., :2], delta[..., 2:].exp() * props[..., 2:]], -1)
        else:
            coord = delta + props
        idx = torch.topk(cls.max(-1)[0], num_queries, dim=1)[1]
        bts.append(torch.gather(coord, 1, idx.unsqueeze(-1).repeat(1, 1, 4)))
        mts.append(torch.gather(y, 1, idx.unsqueeze(-1).repeat(1, 1, d)))
    boxes = torch.cat(bts, 1)
    return boxes.detach(), torch.cat(mts, 1), boxes
