"""GPU: lwdetr_amd.ops.decoder_train on a stand-in with the reference's attribute names.
  - grouped_self_attention against the float64 split / cat formulation of transformer.py:484-495 (output and the gradients of tgt, query_pos
    and every parameter); perturbing one group's rows leaves every other group's output bit-identical;
  - decoder_forward (two layers; one and two levels; image 1 padded) against a float64 restatement: hs, the references, the gradients of tgt,
    memory, the reference points and every parameter;
  - patch_decoder returns 1, keeps the state-dict keys, and the patched stand-in gives the bits of decoder_forward.
Yardstick: figure(got, ref64) <= MARGIN x max(figure of the same restatement run in float32 on the CPU, 2^-24); both figures are printed.
"""
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import two_stage_ref as R
from oracle import lwdetr_torch as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24


class StandInMHA(nn.Module):
    def __init__(self, d, heads):
        super().__init__()
        self.embed_dim, self.num_heads, self.dropout = d, heads, 0.0
        self.in_proj_weight = nn.Parameter(torch.randn(3 * d, d) * d ** -0.5)
        self.in_proj_bias = nn.Parameter(torch.randn(3 * d) * 0.1)
        self.out_proj = nn.Linear(d, d)


class StandInMLP(nn.Module):
    def __init__(self, i, h, o, n):
        super().__init__()
        dims = [i] + [h] * (n - 1) + [o]
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))


class StandInLayer(nn.Module):
    def __init__(self, d, sa_heads, ca_heads, ffn, L, P, groups):
        super().__init__()
        from lwdetr_amd.ops import MSDeformAttnTrain
        self.self_attn = StandInMHA(d, sa_heads)
        self.cross_attn = MSDeformAttnTrain(d, n_levels=L, n_heads=ca_heads, n_points=P)
        self.linear1, self.linear2 = nn.Linear(d, ffn), nn.Linear(ffn, d)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d), nn.LayerNorm(d), nn.LayerNorm(d)
        self.dropout, self.dropout1, self.dropout2, self.dropout3 = (nn.Dropout(0.0) for _ in range(4))
        self.activation, self.group_detr = F.relu, groups


class StandInDecoder(nn.Module):
    def __init__(self, d, sa_heads, ca_heads, ffn, L, P, groups, layers=2):
        super().__init__()
        self.layers = nn.ModuleList(StandInLayer(d, sa_heads, ca_heads, ffn, L, P, groups) for _ in range(layers))
        self.norm = nn.LayerNorm(d)
        self.ref_point_head = StandInMLP(2 * d, d, d, 2)
        self.d_model, self.num_layers = d, layers
        self.lite_refpoint_refine = self.bbox_reparam = self.return_intermediate = True
        self.bbox_embed, self._export = None, False


def randomise(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in module.named_parameters():
            if p.dim() == 1 and "norm" in n and n.endswith("weight"):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=g))
            elif p.dim() == 1:
                p.copy_(0.3 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
    return module


def sa_reference(sa, tgt, query_pos, groups):
    """transformer.py:484-495 with a materialised-softmax MultiheadAttention, in the inputs' dtype."""
    B, Qt, d = tgt.shape
    nq = Qt // groups
    q = k = tgt + query_pos
    v = tgt
    q, k, v = (torch.cat(t.split(nq, dim=1), dim=0) for t in (q, k, v))
    W, b = sa.in_proj_weight, sa.in_proj_bias
    q, k, v = F.linear(q, W[:d], b[:d]), F.linear(k, W[d:2 * d], b[d:2 * d]), F.linear(v, W[2 * d:], b[2 * d:])
    hd = d // sa.num_heads
    sp = lambda t: t.reshape(t.shape[0], nq, sa.num_heads, hd).transpose(1, 2)
    att = ((sp(q) / math.sqrt(hd)) @ sp(k).transpose(-2, -1)).softmax(-1)
    o = sa.out_proj((att @ sp(v)).transpose(1, 2).reshape(-1, nq, d))
    return torch.cat(o.split(B, dim=0), dim=1)


def grads_of(outs, cots, leaves):
    loss = sum((o * c.to(o.dtype).to(o.device)).sum() for o, c in zip(outs, cots))
    return torch.autograd.grad(loss, leaves, allow_unused=True)


def compare(got, ref64, ref32, what):
    fails = []
    for k in ref64:
        f_got, f_yard = R.figure(got[k].detach().cpu(), ref64[k].detach()), R.figure(ref32[k].detach(), ref64[k].detach())
        bound = R.MARGIN * max(f_yard, U32)
        print(f"{what} {k}: figure {f_got:.3e}, float32 restatement {f_yard:.3e}, bound {bound:.3e}")
        if not f_got <= bound:
            fails.append((k, f_got, bound))
    return fails


SA_CASES = [(2, 3, 5, 256, 8), (1, 13, 20, 384, 12), (1, 1, 17, 256, 8)]


def sa_run(sa, tgt, qpos, go, groups, fn):
    t, p = tgt.clone().requires_grad_(True), qpos.clone().requires_grad_(True)
    out = fn(sa, t, p, groups)
    params = dict(sa.named_parameters())
    g = grads_of([out], [go], [t, p] + list(params.values()))
    res = dict(out=out.detach(), g_tgt=g[0], g_query_pos=g[1])
    res.update({"g_" + n: v for n, v in zip(params, g[2:])})
    return res


@pytest.mark.parametrize("case", SA_CASES, ids=lambda c: "x".join(map(str, c)))
def test_grouped_self_attention_against_fp64(case):
    from lwdetr_amd import _native
    from lwdetr_amd.ops import grouped_self_attention
    B, G, nq, d, heads = case
    gen = torch.Generator().manual_seed(sum(case))
    sa = randomise(StandInMHA(d, heads), 3)
    tgt, qpos, go = (torch.randn(B, G * nq, d, generator=gen) for _ in range(3))
    ref64 = sa_run(sa.double(), tgt.double(), qpos.double(), go, G, sa_reference)
    ref32 = sa_run(sa.float(), tgt, qpos, go, G, sa_reference)
    before = _native.attn_train_path_counts()
    sa = sa.to(DEV)
    got = sa_run(sa, tgt.to(DEV), qpos.to(DEV), go, G, grouped_self_attention)
    after = _native.attn_train_path_counts()
    assert sum(after.values()) - sum(before.values()) >= 2, "the fused forward and the fused backward served"
    assert not compare(got, ref64, ref32, f"self-attention {case}")
    if G > 1:                                       # the group is an index: another group's rows do not reach this group's output
        t2 = tgt.clone()
        t2[:, nq:2 * nq] += 1.0
        with torch.no_grad():
            a = grouped_self_attention(sa, tgt.to(DEV), qpos.to(DEV), G)
            b = grouped_self_attention(sa, t2.to(DEV), qpos.to(DEV), G)
        keep = torch.ones(G * nq, dtype=torch.bool)
        keep[nq:2 * nq] = False
        assert torch.equal(a[:, keep], b[:, keep]) and not torch.equal(a[:, ~keep], b[:, ~keep])


def decoder_reference(dec, tgt, memory, refpoints, level_shapes, valid_ratios, mask, groups):
    """transformer.py:328-427 / 466-517 restated functionally (split / cat self-attention, grid_sample sampling), in the inputs' dtype."""
    d = dec.d_model
    ref_in = refpoints[:, :, None] * torch.cat([valid_ratios, valid_ratios], -1)[:, None]
    qpos = ref_in[:, :, 0, :]
    qpos = O.sine_embed(qpos, d // 2)
    qpos = dec.ref_point_head.layers[1](F.relu(dec.ref_point_head.layers[0](qpos)))
    x, hs = tgt, []
    for lay in dec.layers:
        x = lay.norm1(x + sa_reference(lay.self_attn, x, qpos, groups))
        ca = lay.cross_attn
        B, Q, _ = x.shape
        query = x + qpos
        value = ca.value_proj(memory).masked_fill(mask[..., None], 0.0)
        off = ca.sampling_offsets(query).view(B, Q, ca.n_heads, ca.n_levels, ca.n_points, 2)
        aw = ca.attention_weights(query).view(B, Q, ca.n_heads, -1).softmax(-1).view(B, Q, ca.n_heads, ca.n_levels, ca.n_points)
        loc = ref_in[:, :, None, :, None, :2] + off / ca.n_points * ref_in[:, :, None, :, None, 2:] * 0.5
        core = O.msda_core(value.view(B, -1, ca.n_heads, d // ca.n_heads), level_shapes, loc, aw)
        x = lay.norm2(x + ca.output_proj(core))
        x = lay.norm3(x + lay.linear2(F.relu(lay.linear1(x))))
        hs.append(dec.norm(x))
    return torch.stack(hs), refpoints.unsqueeze(0)


def decoder_inputs(levels, B, G, nq, d, seed):
    gen = torch.Generator().manual_seed(seed)
    S = sum(h * w for h, w in levels)
    tgt, memory = torch.randn(B, G * nq, d, generator=gen), torch.randn(B, S, d, generator=gen)
    ref = torch.cat([torch.rand(B, G * nq, 2, generator=gen) * 0.8 + 0.1, torch.rand(B, G * nq, 2, generator=gen) * 0.4 + 0.05], -1)
    masks, ratios = [], []
    for h, w in levels:
        m = torch.zeros(B, h, w, dtype=torch.bool)
        m[1, :, max(1, (w * 2) // 3):] = True                      # image 1 is padded on the right and at the bottom
        m[1, max(1, (h * 3) // 4):, :] = True
        masks.append(m.flatten(1))
        ratios.append(torch.stack([(~m[:, 0, :]).sum(1).float() / w, (~m[:, :, 0]).sum(1).float() / h], -1))
    go_hs = torch.randn(2, B, G * nq, d, generator=gen)
    go_ref = torch.randn(1, B, G * nq, 4, generator=gen)
    return dict(tgt=tgt, memory=memory, ref=ref, mask=torch.cat(masks, 1), vr=torch.stack(ratios, 1), go=(go_hs, go_ref))


def decoder_run(dec, inp, levels, groups, ct, device, fn):
    t = lambda k: inp[k].to(device=device, dtype=ct).clone().requires_grad_(True)
    tgt, memory, ref = t("tgt"), t("memory"), t("ref")
    hs, refs = fn(dec, tgt, memory, ref, levels, inp["vr"].to(device=device, dtype=ct), inp["mask"].to(device), groups)
    params = dict(dec.named_parameters())
    g = grads_of([hs, refs], inp["go"], [tgt, memory, ref] + list(params.values()))
    res = dict(hs=hs.detach(), references=refs.detach(), g_tgt=g[0], g_memory=g[1], g_refpoints=g[2])
    res.update({"g_" + n: v for n, v in zip(params, g[2 + 1:])})
    return res


def fused_call(dec, tgt, memory, ref, levels, vr, mask, groups):
    from lwdetr_amd.ops import decoder_forward
    shapes = torch.as_tensor(levels, dtype=torch.long, device=tgt.device)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    return decoder_forward(dec, tgt, memory, ref, shapes, lsi, vr, mask, groups)


DEC_CASES = [pytest.param([(6, 5)], 2, id="one-level"), pytest.param([(8, 6), (4, 3)], 4, id="two-levels")]


@pytest.mark.parametrize("levels,points", DEC_CASES)
def test_decoder_forward_against_fp64(levels, points):
    from lwdetr_amd import _native
    B, G, nq, d = 2, 3, 7, 256
    dec = randomise(StandInDecoder(d, 8, 16, 64, len(levels), points, G), 11).train()
    inp = decoder_inputs(levels, B, G, nq, d, 5)
    ref64 = decoder_run(dec.double(), inp, levels, G, torch.float64, "cpu", decoder_reference)
    ref32 = decoder_run(dec.float(), inp, levels, G, torch.float32, "cpu", decoder_reference)
    counts = [_native.attn_train_path_counts, _native.msda_train_path_counts, _native.train_glue_path_counts]
    before = [sum(c().values()) for c in counts]
    got = decoder_run(dec.to(DEV), inp, levels, G, torch.float32, DEV, fused_call)
    torch.cuda.synchronize()
    delta = [sum(c().values()) - b for c, b in zip(counts, before)]
    assert delta[0] >= 4 and delta[1] >= 4 and delta[2] == 2, f"fused launches (attention, deformable attention, sine embed): {delta}"
    assert got["hs"].shape == (2, B, G * nq, d) and got["references"].shape == (1, B, G * nq, 4)
    assert not compare(got, ref64, ref32, f"decoder {levels}")


def test_patch_decoder_binds_decoder_forward():
    from lwdetr_amd.ops import patch_decoder
    levels, B, G, nq, d = [(8, 6), (4, 3)], 2, 3, 7, 256
    dec = randomise(StandInDecoder(d, 8, 16, 64, 2, 4, G), 11).to(DEV).train()
    holder = nn.Module()
    holder.decoder = dec
    keys = set(holder.state_dict())
    inp = decoder_inputs(levels, B, G, nq, d, 5)
    t = lambda k: inp[k].to(DEV)
    shapes = torch.as_tensor(levels, dtype=torch.long, device=DEV)
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    with torch.no_grad():
        want_hs, want_ref = fused_call(dec, t("tgt"), t("memory"), t("ref"), levels, t("vr"), t("mask"), G)
        assert patch_decoder(holder) == 1 and set(holder.state_dict()) == keys
        hs, refs = dec(t("tgt"), t("memory"), memory_key_padding_mask=t("mask"), pos=None, refpoints_unsigmoid=t("ref"), level_start_index=lsi,
                       spatial_shapes=shapes, valid_ratios=t("vr"))
        assert torch.equal(hs, want_hs) and torch.equal(refs, want_ref)
        dec.eval()                                   # one group in eval mode: the first group's queries alone
        hs1, _ = dec(t("tgt")[:, :nq], t("memory"), memory_key_padding_mask=t("mask"), refpoints_unsigmoid=t("ref")[:, :nq], level_start_index=lsi,
                     spatial_shapes=shapes, valid_ratios=t("vr"))
        assert hs1.shape == (2, B, nq, d)
    dec.train()
    dec.layers[0].dropout1.p = 0.1
    with pytest.raises(NotImplementedError):
        dec(t("tgt"), t("memory"), memory_key_padding_mask=t("mask"), refpoints_unsigmoid=t("ref"), level_start_index=lsi, spatial_shapes=shapes,
            valid_ratios=t("vr"))
