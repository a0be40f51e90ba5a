"""GPU: the selection kernels of csrc/topk.hip and the two row kernels of the decoder set-up at the shapes where their code forks.

lwdetr_topk / lwdetr_postprocess*: the first digit of the radix select is taken from the top bits of key - smallest key, the winners are bucketed by
it and the threshold bin's elements ranked as a candidate list (heavy ties: digit passes), the block size follows N, the loads are 16-byte
vectors behind a scalar head. So: keys clustered in a few binades (the
distribution of detection logits), keys spread over 24 binades with +-inf and +-0, one key apart from N - 1 equal ones, keys that differ in the last
mantissa bit only, N around the vector and block edges with bases that are only element-aligned, a threshold inside a tie larger than the block,
and an input too large for the LDS key cache. The expectation is a stable descending sort on the host of the kernel's own order (the monotone integer
image of the float, which orders +0 above -0; equal keys by ascending index) - for inputs without signed zeros that is torch.sort(stable=True).

lwdetr_select_gather / lwdetr_decoder_inputs: several rows per workgroup, 16-byte accesses where the bases allow. Gather is compared exactly;
decoder_inputs bit for bit with what the one-workgroup-per-row kernels wrote (tests/golden/select_rows_parent.npz, recorded once on an MI355X from
the inputs generated below). Every output sits between guard rows that must keep their sentinel.
"""
import functools
import os

import numpy as np
import pytest
import torch

import lwdetr_amd
import lwdetr_amd.models
from lwdetr_amd import _native

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "select_rows_parent.npz")
SENT = 1234.0
TK_CACHE_BYTES_MAX = 160 * 1024            # csrc/topk.hip: the key cache is what is left of 160 KB, so N * 4 = 160 KB is past it


def _name(dt):
    return str(dt).split(".")[-1]


# ---------------------------------------------------------------------------------------------------------------- top-k plumbing
def _topk_raw(x, k, off=0):
    """x (B, N) host tensor -> (val, idx) of lwdetr_topk; the device copy starts `off` elements past a 256-byte aligned allocation."""
    b, n = x.shape
    buf = torch.zeros(b * n + off + 16, dtype=x.dtype, device=DEV)
    buf[off:off + b * n] = x.flatten().to(DEV)
    idx = torch.full((b, k), -7, dtype=torch.int64, device=DEV)
    val = torch.full((b, k), float("nan"), dtype=torch.float32, device=DEV)
    rc = _native.lib().lwdetr_topk(buf.data_ptr() + off * buf.element_size(), b, n, k, idx.data_ptr(), val.data_ptr(), _native.dtype_code(x.dtype),
                                   _native.stream_ptr(DEV))
    _native.check(rc, "lwdetr_topk")
    return val.cpu(), idx.cpu()


def _order_key(x):
    """Monotone integer image of the float (the kernel's order): ascending, -0 just below +0."""
    bits = x.float().contiguous().numpy().view(np.uint32).astype(np.int64)
    return np.where(bits & 0x80000000, 0xFFFFFFFF - bits, bits | 0x80000000)


def _expected(x, k):
    key = _order_key(x)
    order = np.argsort(-key, axis=1, kind="stable")[:, :k]
    return torch.from_numpy(np.take_along_axis(x.float().numpy(), order, 1)), torch.from_numpy(order)


def _check_topk(x, k, off=0):
    val, idx = _topk_raw(x, k, off)
    ev, ei = _expected(x, k)
    assert torch.equal(idx, ei), f"indices differ at {int((idx != ei).sum())} of {idx.numel()} places"
    assert torch.equal(val.view(torch.int32), ev.view(torch.int32))            # bit for bit: the sign of a zero included


def _clustered(shape, g):
    return (-4.6 + 0.8 * torch.randn(shape, generator=g)).to(F16).float()


def _wide(shape, g):
    x = torch.randn(shape, generator=g) * torch.pow(2.0, torch.randint(-12, 12, shape, generator=g).float())
    x[..., 3::29] = float("inf")
    x[..., 5::31] = float("-inf")
    x[..., 7::13] = 0.0
    x[..., 2::17] = -0.0
    return x


# ---------------------------------------------------------------------------------------------------------------- top-k cases
@pytest.mark.parametrize("dtype", [F32, F16], ids=_name)
@pytest.mark.parametrize("n", [1600, 27300])
@pytest.mark.parametrize("kind", ["clustered", "all_but_one_low", "all_but_one_high", "last_bit", "wide"])
def test_topk_key_distributions(kind, n, dtype):
    """(B 3, N, K 300). all_but_one_*: min == max over all but one element, the odd one below / above (inside the winners) - the common prefix of
    min and max is then decided by a single key. last_bit: two values one ulp of `dtype` apart."""
    g = torch.Generator().manual_seed(n + len(kind))
    b, k = 3, 300
    if kind == "clustered":
        x = _clustered((b, n), g)
    elif kind.startswith("all_but_one"):
        x = torch.full((b, n), -4.59375)
        x[:, n // 3] = -7.5 if kind.endswith("low") else -0.5
        x[1, n // 3], x[1, n - 1] = -4.59375, (-4.6015625 if kind.endswith("low") else -4.5859375)     # a neighbouring f16 value: differs in the low bits only
    elif kind == "last_bit":
        lo = torch.tensor(-4.59375)
        hi = torch.nextafter(lo.to(dtype), torch.tensor(0.0, dtype=dtype)).float() if dtype == F32 else torch.tensor(-4.58984375)
        assert float(hi) > float(lo) and float(hi.to(dtype)) == float(hi)
        x = torch.where(torch.rand(b, n, generator=g) < 0.4, hi, lo)
    else:
        x = _wide((b, n), g)
    _check_topk(x.to(dtype), k)


@pytest.mark.parametrize("dtype", [F16, F32], ids=_name)
@pytest.mark.parametrize("n", [1, 7, 9, 255, 257, 1023, 1025, 2049])
def test_topk_sizes_at_vector_and_block_edges(n, dtype):
    """B = 3 images of N elements back to back: with odd N the second image starts on an element boundary only; every case again with the whole input
    moved one element off its 16-byte boundary. K = 1, min(N, 300), N (K <= 1024)."""
    g = torch.Generator().manual_seed(n)
    x = _clustered((3, n), g).to(dtype)
    for k in sorted({1, min(n, 300), n}):
        if k > 1024:
            continue
        for off in (0, 1):
            _check_topk(x, k, off)
    xw = _wide((3, n), g).to(dtype)
    _check_topk(xw, min(n, 300), 1)


@pytest.mark.parametrize("n", [4000, 8192])
def test_topk_threshold_inside_a_large_tie(n):
    """Four levels: each holds N / 4 elements, more than the block has threads (512 at N = 4000, 1024 at N = 8192) and more than the candidate list
    holds, and the 300th value lies inside one: the index order alone decides which of its elements are taken."""
    g = torch.Generator().manual_seed(n)
    x = torch.randint(0, 4, (3, n), generator=g).float() * 0.25 - 5.0
    assert int((x[0] == x[0].max()).sum()) > (512 if n == 4000 else 1024)
    _check_topk(x, 300)
    _check_topk(x, min(1024, n // 4 + 100))                                       # the threshold inside the second level


def test_topk_uncached_path():
    """N * 4 = 160 KB is past the key cache: the passes re-read global memory."""
    n = 40960
    assert n * 4 >= TK_CACHE_BYTES_MAX
    g = torch.Generator().manual_seed(n)
    _check_topk(_clustered((2, n), g), 300)
    _check_topk(_wide((2, n), g), 300, off=1)


# ---------------------------------------------------------------------------------------------------------------- PostProcess
def _postprocess_expected(logits, boxes, sizes, k, dtype):
    b, nq, c = logits.shape
    lv, li = _expected(logits.view(b, -1), k)
    es = lv.sigmoid().to(dtype).float()
    cx, cy, w, h = boxes.unbind(-1)
    w, h = w.clamp(min=0), h.clamp(min=0)
    xyxy = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], -1)          # in `dtype`, as the reference
    exy = torch.gather(xyxy, 1, (li // c).unsqueeze(-1).repeat(1, 1, 4)).float()
    exy = exy * torch.stack([sizes[:, 1], sizes[:, 0], sizes[:, 1], sizes[:, 0]], 1)[:, None, :]
    return es, li % c, exy


@pytest.mark.parametrize("dtype", [F16, F32], ids=_name)
@pytest.mark.parametrize("b_nq_c_k", [(2, 300, 91, 300), (1, 7, 3, 5)], ids=lambda s: "x".join(map(str, s)))
def test_postprocess_clustered_logits_both_entries(dtype, b_nq_c_k):
    """Against the reference's tensor ops with the tie order made explicit, as tests/test_gpu_topk.py does; the packed entry carries the same values."""
    b, nq, c, k = b_nq_c_k
    g = torch.Generator().manual_seed(c + k)
    logits = _clustered((b, nq, c), g).to(dtype)
    boxes = torch.rand(b, nq, 4, generator=g).to(dtype)
    boxes[:, ::3, 2] = -0.05                      # negative widths are clamped
    sizes = torch.tensor([[480.0, 640.0], [333.0, 500.0]])[:b]
    post = lwdetr_amd.models.PostProcess(k)
    s, l, bx = post.select(logits.to(DEV), boxes.to(DEV), sizes.to(DEV))
    es, el, exy = _postprocess_expected(logits, boxes, sizes, k, dtype)
    ulp = {F32: 5e-7, F16: 1e-3}[dtype]
    assert s.shape == (b, k) and l.dtype == torch.int64 and bx.shape == (b, k, 4)
    assert (s.cpu() - es).abs().max().item() <= ulp
    assert torch.equal(l.cpu(), el)
    assert (bx.cpu() - exy).abs().max().item() <= ulp * 1300
    from lwdetr_amd.dist import pack_detections
    packed = post.select_packed(logits.to(DEV), boxes.to(DEV), sizes.to(DEV))
    assert packed.shape == (b, k, 6) and torch.equal(packed, pack_detections(s, l, bx))


def test_topk_and_postprocess_graph_replay_is_bit_identical_to_eager():
    g = torch.Generator().manual_seed(11)
    b, n, k, nq, c = 2, 1600, 300, 300, 91
    x = _clustered((b, n), g).to(DEV)
    logits = _clustered((b, nq, c), g).to(F16).to(DEV)
    boxes = torch.rand(b, nq, 4, generator=g).to(F16).to(DEV)
    sizes = torch.tensor([[480.0, 640.0], [333.0, 500.0]], device=DEV)
    idx = torch.empty(b, k, dtype=torch.int64, device=DEV)
    val = torch.empty(b, k, dtype=torch.float32, device=DEV)
    packed = torch.empty(b, k, 6, dtype=torch.float32, device=DEV)
    L = _native.lib()

    def run():
        st = _native.stream_ptr(DEV)
        _native.check(L.lwdetr_topk(x.data_ptr(), b, n, k, idx.data_ptr(), val.data_ptr(), 0, st), "lwdetr_topk")
        _native.check(L.lwdetr_postprocess_packed(logits.data_ptr(), boxes.data_ptr(), sizes.data_ptr(), b, nq, c, k, packed.data_ptr(), 1, st),
                      "lwdetr_postprocess_packed")

    run()
    torch.cuda.synchronize()
    eager = [t.clone() for t in (idx, val, packed)]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    for t in (idx, val, packed):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, e) for a, e in zip((idx, val, packed), eager))
    ev, ei = _expected(x.cpu(), k)
    assert torch.equal(idx.cpu(), ei)


# ---------------------------------------------------------------------------------------------------------------- row kernels
ROW_CASES = {"b2s50": (2, 50, 256, 5, 91, 96), "b1s9": (1, 9, 256, 9, 3, 4)}     # B, S, d, nq, ncls, ldc
ROW_DTYPES = [F16, F32]
ROW_L = 3


class Out:
    """rows x ld elements of `dtype` between two guard rows on either side, everything filled with the sentinel. The body starts on a 16-byte
    boundary plus `off` elements."""

    def __init__(self, rows, ld, dtype, off):
        self.rows, self.ld = rows, ld
        self.start = -(-2 * ld // 8) * 8 + off
        self.buf = torch.full((self.start + rows * ld + 2 * ld + 8,), SENT, dtype=dtype, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.ptr = self.buf.data_ptr() + self.start * self.buf.element_size()

    def body(self):
        """The body on the host; asserts that nothing outside it was written."""
        torch.cuda.synchronize()
        h = self.buf.cpu()
        n = self.rows * self.ld
        sent = torch.tensor(SENT).to(h.dtype)
        assert bool((h[:self.start] == sent).all()) and bool((h[self.start + n:] == sent).all()), "a guard element was overwritten"
        return h[self.start:self.start + n].view(self.rows, self.ld)


def _shifted(t, off):
    """A device copy of t whose first element sits `off` elements past a 16-byte boundary; (tensor kept alive, address)."""
    buf = torch.zeros(t.numel() + off + 8, dtype=t.dtype, device=DEV)
    buf[off:off + t.numel()] = t.flatten().to(DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + off * buf.element_size()


@functools.lru_cache(maxsize=None)
def decoder_case(case, dtype):
    """Seeded inputs of lwdetr_decoder_inputs (host tensors): exp arguments in [-4, 1.5], widths up to ~8, sine arguments of tens of radians."""
    B, S, d, nq, ncls, ldc = ROW_CASES[case]
    g = torch.Generator().manual_seed(1000 * nq + d + B)
    n = B * nq
    enc_delta = torch.cat([torch.randn(n, 2, generator=g) * 0.5, torch.rand(n, 2, generator=g) * 5.5 - 4], 1)
    enc_delta[0, 2], enc_delta[0, 3] = 1.5, -4.0
    enc_delta = enc_delta.to(dtype)
    props = torch.cat([torch.rand(n, 2, generator=g), torch.rand(n, 2, generator=g) * 0.35 + 0.05], 1)
    refpoint = torch.cat([torch.randn(nq, 2, generator=g) * 1.5, torch.rand(nq, 2, generator=g) * 5.5 - 4], 1)
    refpoint[0, 2], refpoint[0, 3] = -4.0, 1.5
    vr = (0.5 + 0.5 * (torch.randperm(B * ROW_L * 2, generator=g).float() + 1) / (B * ROW_L * 2 + 1)).view(B, ROW_L, 2)
    query = torch.randn(nq, d, generator=g).to(dtype)
    dim_t = (10000 ** (2 * (torch.arange(d // 2, dtype=torch.float32) // 2) / (d // 2))).contiguous()
    return enc_delta, props, refpoint, vr, query, dim_t


def run_decoder_inputs(case, dtype, off):
    """-> dict of the four outputs (host tensors). `off` shifts every 16-bit / 32-bit row base (inputs and outputs) off its 16-byte boundary."""
    B, S, d, nq, ncls, ldc = ROW_CASES[case]
    n = B * nq
    keep = [_shifted(t, off) for t in decoder_case(case, dtype)]
    outs = dict(enc_boxes=Out(n, 4, dtype, off), ref=Out(n, 4, F32, off), sine=Out(n, 2 * d, dtype, off), xdec=Out(n, d, dtype, off))
    p = [a for _, a in keep]
    rc = _native.lib().lwdetr_decoder_inputs(p[0], p[1], p[2], p[3], ROW_L, p[4], p[5], outs["enc_boxes"].ptr, outs["ref"].ptr, outs["sine"].ptr,
                                             outs["xdec"].ptr, B, nq, d, _native.dtype_code(dtype), _native.stream_ptr(DEV))
    _native.check(rc, "lwdetr_decoder_inputs")
    return {k: v.body() for k, v in outs.items()}


def golden_key(case, dtype, name):
    return f"{case}_{_name(dtype)}_{name}"


def as_bytes(t):
    return t.contiguous().view(torch.uint8).numpy()


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("dtype", ROW_DTYPES, ids=_name)
@pytest.mark.parametrize("case", list(ROW_CASES))
def test_decoder_inputs_bit_identical_to_the_row_per_workgroup_kernel(case, dtype, off):
    gold = np.load(GOLDEN)
    got = run_decoder_inputs(case, dtype, off)
    B, S, d, nq, ncls, ldc = ROW_CASES[case]
    assert torch.equal(got["xdec"], decoder_case(case, dtype)[4].repeat(B, 1))
    for name, t in got.items():
        exp = gold[golden_key(case, dtype, name)]
        assert np.array_equal(as_bytes(t), exp), f"{name}: {int((as_bytes(t) != exp).sum())} bytes differ"


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "shifted"])
@pytest.mark.parametrize("dtype", [F16, BF16, F32], ids=_name)
@pytest.mark.parametrize("case", list(ROW_CASES))
def test_select_gather_exact(case, dtype, off):
    B, S, d, nq, ncls, ldc = ROW_CASES[case]
    g = torch.Generator().manual_seed(S + nq)
    idx = torch.randint(0, S, (B, nq), generator=g)
    idx[:, 0], idx[:, -1] = 0, S - 1
    idx[:, 1] = idx[:, 2]                                       # a duplicate
    flat = (torch.arange(B)[:, None] * S + idx).flatten()
    om = torch.randn(B * S, d, generator=g).to(dtype)
    enc_cls = torch.randn(B * S, ldc, generator=g).to(dtype)
    enc_cls[:, ncls:] = 7777.0                                  # pad columns: never copied
    props = torch.rand(B * S, 4, generator=g)
    n = B * nq
    keep = [_shifted(t, off) for t in (om, enc_cls, props)] + [_shifted(idx, 0)]
    om_sel, logits, props_sel = Out(n, d, dtype, off), Out(n, ncls, dtype, off), Out(n, 4, F32, off)
    rc = _native.lib().lwdetr_select_gather(keep[0][1], keep[1][1], ldc, keep[2][1], keep[3][1], om_sel.ptr, logits.ptr, props_sel.ptr, B, S, d, nq,
                                            ncls, _native.dtype_code(dtype), _native.stream_ptr(DEV))
    _native.check(rc, "lwdetr_select_gather")
    assert torch.equal(om_sel.body(), om[flat])
    assert torch.equal(logits.body(), enc_cls[flat, :ncls])
    assert torch.equal(props_sel.body(), props[flat])
