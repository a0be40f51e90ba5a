"""The element bounds of tests/test_gpu_chain_fp64.py, met on the CPU by a correct implementation other than the code under test, and a model of the
weight ring's accounting.

(1) An independent FLOAT32 emulation of the chain.hip arithmetic in numpy. It does not use the float64 reference's dense weights: it walks the PACKED
    stream fragment by fragment as the kernels do (global fragment g = 4 piece + f is the 1 KB at g * 1024 bytes, lane 32 h + i holds output channel i,
    k-slots 8 h .. 8 h + 7; as tests/chain_sim.py, one 16-slot MFMA step after the other in f32), hands accumulator tiles on in k-slot order by its own
    formula, and rounds to the storage type where the kernels do. It stays inside the worst-case bound on every element of every case the GPU module
    launches and outside the tight bound on no more than SHARE of a tensor, with the committed seeds.
(2) Each of a list of planted mistakes in that emulation fails the comparison: an element outside the worst-case bound, or more than SHARE of a
    tensor outside the tight one.
(3) A Python model of WRing's accounting (fill, begin_tile, begin_tile_x with seq_of, the split kernel's begin_group) over every chain description the
    GPU module launches and a sweep of all stage programs of up to 3 stages: every fragment read (the CH_RD read-ahead included) hits a slot whose DMA
    was issued and is covered by the modelled wait, no slot is refilled before the barrier that follows its last read, no read goes beyond piece
    np - 1. A shape that would read an unfilled slot or wait for a DMA that was never issued is found here, not on a GPU."""
import itertools

import numpy as np
import pytest
import torch

from tests import test_gpu_chain_fp64 as G
from tests.test_gpu_rowops import F16, BF16

f32 = np.float32
CH_RD = 8


def _r(v, T):
    """f32 array -> nearest T, as f32."""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=f32)).to(T).float().numpy()


def slot_channels(D):
    """Channel held by k-slot p = 16 t + 8 h + e of an accumulator tile handed on as a B operand: fragment t = 2 n + beta holds registers 8 beta + e
    of tile n, register r of lane (j, h) is channel 32 n + 8 (r / 4) + 4 h + r % 4 (chain.hip: `xf[2 * n] = w[0..3], xf[2 * n + 1] = w[4..7]`)."""
    out = []
    for p in range(D):
        t, rem = divmod(p, 16)
        h, e = divmod(rem, 8)
        n, beta = divmod(t, 2)
        r = 8 * beta + e
        out.append(32 * n + 8 * (r // 4) + 4 * h + r % 4)
    return np.array(out)


class Stream:
    def __init__(self, stream):
        self.frags = stream.float().numpy().reshape(-1, 64, 8)

    def tile(self, X, g0, nf, start, two=False, x0=0):
        """32 output channels: nf fragments from global fragment g0 against the operand slots [16 x0, 16 (x0 + nf)) of X (rows, K), on top of start."""
        F = self.frags[g0:g0 + nf].reshape(nf, 2, 32, 8).transpose(2, 0, 1, 3).reshape(32, nf * 16)
        acc = np.broadcast_to(start.astype(f32), (X.shape[0], 32)).copy()
        acc2 = np.zeros_like(acc)
        for f in range(nf):
            part = X[:, 16 * (x0 + f):16 * (x0 + f) + 16] @ F[:, 16 * f:16 * f + 16].T
            if two and (f & 1):
                acc2 = acc2 + part
            else:
                acc = acc + part
        return acc + acc2 if two else acc


def _ln(v, gam, bet, eps, wrong=None):
    """Two-pass f32 statistics of the rounded rows; fmaf((v - mean) rstd, g, b): one rounding (evaluated in float64, rounded to f32)."""
    D = v.shape[1]
    mean = v.sum(1, keepdims=True, dtype=f32) * f32(1.0 / D)
    d = v - mean
    rstd = f32(1.0) / np.sqrt((d * d).sum(1, keepdims=True, dtype=f32) * f32(1.0 / D) + f32(eps))
    if wrong == "gamma / beta exchanged":
        gam, bet = bet, gam
    return ((d * rstd).astype(np.float64) * gam.astype(np.float64) + bet.astype(np.float64)).astype(f32)


def emu_row(case, split, wrong=None):
    """mlp_chain_kernel (split False) / mlp_chain_split_kernel (True) in f32: {stage: stored rows (M, n)}."""
    D, T, k_in, M = case["D"], case["T"], case["k_in"], case["M"]
    S, vec, chan = Stream(case["stream"]), case["vec"].numpy().astype(f32), slot_channels(D)
    PPT, KS = D // 64, D // 16
    halves = 2 if D == 384 else 1
    assert split or D == 256
    X = case["x"].float().numpy()
    res = case["res"].float().numpy() if case["res"] is not None else None
    q = case["qpos"].float().numpy() if case["qpos"] is not None else None
    if wrong == "residual rows 8 off" and res is not None:
        res = np.roll(res, 8, axis=0)
    pc, off, outs = 0, 0, {}

    def tiles(X, nt, K_, start_of):
        """nt tiles of 32 channels in stream order: tile after tile, or (D = 384) k-half-major inside groups of 4."""
        nonlocal pc
        cols = []
        if halves == 1:
            for n in range(nt):
                cols.append(S.tile(X, 4 * pc, K_ // 16, start_of(n), two=split))
                pc += K_ // 64
            return np.concatenate(cols, 1)
        KSH, PPH = KS // 2, PPT // 2
        for g0 in range(0, nt, 4):
            ng = min(4, nt - g0)
            for w in range(ng):
                h0, h1 = (1, 0) if wrong == "k-halves exchanged" else (0, 1)
                a = S.tile(X, 4 * (pc + w * PPH), KSH, start_of(g0 + w), two=True, x0=h0 * KSH)
                cols.append(S.tile(X, 4 * (pc + ng * PPH + w * PPH), KSH, a, two=True, x0=h1 * KSH))
            pc += 2 * ng * PPH
        return np.concatenate(cols, 1)

    for i, st in enumerate(case["stages"]):
        if st["kind"] == "side":
            nt = (st["n"] + 31) // 32
            b = vec[off:off + 32 * nt]
            off += 32 * nt
            outs[i] = _r(tiles(X, nt, D, lambda n: b[32 * n:32 * n + 32]), T)[:, :st["n"]]
            continue
        b = vec[off:off + D]
        off += D
        if st.get("ln") is not None:
            gam, bet = vec[off:off + D], vec[off + D:off + 2 * D]
            off += 2 * D
        if wrong == "bias of the neighbouring tile":
            b = np.roll(b, 32)
        start = (lambda n: b[32 * n:32 * n + 32] + res[:, 32 * n:32 * n + 32]) if st.get("res") else (lambda n: b[32 * n:32 * n + 32])
        pre = tiles(X, D // 32, k_in if i == 0 else D, start)
        if st.get("relu"):
            pre = np.abs(_r(pre, T)) if wrong == "ReLU after rounding with a sign flip" else np.maximum(pre, f32(0))
        y = pre if wrong == "unrounded hand-over" else _r(pre, T)
        if st.get("ln") is not None:
            y = _ln(y, gam, bet, st["ln"], wrong)
            y = y if wrong == "unrounded hand-over" else _r(y, T)
        nxt = _r(y + q, T) if st.get("addq") else y
        if st.get("store"):
            outs[i] = _r(nxt if wrong == "the stored row includes qpos" else y, T)
        X = nxt[:, chan]
    assert pc + 2 == S.frags.shape[0] // 4
    return {i: torch.from_numpy(v).double() for i, v in outs.items()}


def emu_enc(case, wrong=None):
    """enc_chain_kernel / enc_chain_kernel_wide in f32: {name: rows at the launch's memory rows}."""
    D, T, k5, nl, cols, ncls, M = case["D"], case["T"], case["k5"], case["nl"], case["cols"], case["ncls"], case["M"]
    S, vec, chan = Stream(case["stream"]), case["vec"].numpy().astype(f32), slot_channels(D)
    NTI, KS = D // 32, D // 16
    two = D == 256 and not k5
    idx = torch.arange(M) if wrong == "a flag indexed by m instead of mm" else case["mm"]
    rv, npd = case["rowvalid"][idx].numpy().astype(f32), case["notpad"][idx].numpy().astype(f32)
    off = 3 * D if k5 else 0
    bes, ges, bts = vec[off:off + D], vec[off + D:off + 2 * D], vec[off + 2 * D:off + 3 * D]
    bcs, bvs = vec[off + 3 * D:off + 3 * D + cols], vec[off + 3 * D + cols:]
    X = case["x"].float().numpy()
    g, out = 0, {}
    if k5:
        acc = []
        for n in range(NTI):
            acc.append(S.tile(X, g, k5 // 16, vec[32 * n:32 * n + 32], two))
            g += k5 // 16
        a = np.concatenate(acc, 1)
        v = _r(a / (f32(1.0) + np.exp(-a)), T)
        mem = _r(_ln(v, vec[D:2 * D], vec[2 * D:3 * D], case["eps_p"], wrong), T)
        out["memory"] = mem
        Xf = mem[:, chan]
    else:
        Xf = X
    vals = []
    for vt in range(nl * NTI):
        b = bvs[32 * vt:32 * vt + 32]
        if wrong == "the mask applied before the bias":
            a = S.tile(Xf, g, KS, np.zeros(32, f32), two) * npd[:, None] + b
        else:
            a = S.tile(Xf, g, KS, b, two) * npd[:, None]
        vals.append(a)
        g += KS
    out["values"] = _r(np.concatenate(vals, 1), T)
    Xe = Xf * rv[:, None]
    acc = []
    for n in range(NTI):
        acc.append(S.tile(Xe, g, KS, bes[32 * n:32 * n + 32], two))
        g += KS
    y = np.concatenate(acc, 1)
    y = y if wrong == "unrounded hand-over" else _r(y, T)
    om = _r(_ln(y, ges, bts, case["eps_e"], wrong), T)
    out["om"] = om
    Xo = om[:, chan]
    acc = []
    for n in range(cols // 32):
        acc.append(S.tile(Xo, g, KS, bcs[32 * n:32 * n + 32], two))
        g += KS
    out["cls"] = _r(np.concatenate(acc, 1), T)
    out["cls_max"] = out["cls"][:, :cols if wrong == "the row maximum over all cols" else ncls].max(1)
    assert g + 8 == S.frags.shape[0]
    return {n: torch.from_numpy(np.ascontiguousarray(v)).double() for n, v in out.items()}


# ------------------------------------------------------------------------------------------------------------ (1) the emulation meets both bounds
def outside(got, ref, T):
    y, e = ref
    return int((~((got - y).abs() <= G.bound_of(y, e, T))).sum())


def check_row(case, split, label):
    got = emu_row(case, split)
    for i, rows in got.items():
        n = rows.shape[1]
        (yt, et), (yw, ew) = case["tight", split][i], case["worst", split][i]
        G.check("host", rows, (yt[:, :n], et[:, :n]), (yw[:, :n], ew[:, :n]), case["T"], f"host {label} stage {i}")


def check_enc(case, label):
    got = emu_enc(case)
    for n in got:
        if n != "cls_max":
            G.check("host", got[n], case["tight"][n], case["worst"][n], case["T"], f"host {label} {n}")
    assert torch.equal(got["cls_max"], got["cls"][:, :case["ncls"]].max(1).values)
    assert bool((got["cls"][:, case["ncls"]:] == 0).all())
    assert bool((got["values"][case["notpad"][case["mm"]] == 0] == 0).all())


@pytest.mark.parametrize("T", [F16, BF16], ids=lambda v: G.NAME[v])
@pytest.mark.parametrize("D", [256, 384])
def test_split_cases_meet_both_bounds_in_f32(D, T):
    for name, M in G.SPLIT_PROGRAMS:
        check_row(G.row_case(name, D, T, M), True, f"split {G.NAME[T]} d{D} {name} M{M}")


@pytest.mark.parametrize("T", [F16, BF16], ids=lambda v: G.NAME[v])
def test_row_per_wave_cases_meet_both_bounds_in_f32(T):
    for name, M, _ in G.ROW_PROGRAMS:
        check_row(G.row_case(name, 256, T, M), False, f"row {G.NAME[T]} {name} M{M}")


@pytest.mark.parametrize("T", [F16, BF16], ids=lambda v: G.NAME[v])
@pytest.mark.parametrize("width", ["narrow", "wide"])
@pytest.mark.parametrize("D,k5", G.ENC_FORMS)
def test_enc_cases_meet_both_bounds_in_f32(D, k5, width, T):
    for M, geo, nl, ci, _, _ in G.ENC_SHAPES:
        ncls = G.NCLS[width][ci]
        check_enc(G.enc_case(D, k5, T, width, M, geo, nl, ncls), f"enc {G.NAME[T]} d{D} k5 {k5} {width} M{M} nl{nl} ncls{ncls}")


@pytest.mark.parametrize("T", [F16, BF16], ids=lambda v: G.NAME[v])
def test_routing_cases_meet_both_bounds_in_f32(T):
    """The cases of test_row_chain_routing_without_the_knob: 16 384 rows in the split form, 16 385 in the row-per-wave form, k_in = 512, D = 384."""
    check_row(G.row_case("side1_4", 256, T, 16384), True, f"routing {G.NAME[T]} M16384")
    check_row(G.row_case("side1_4", 256, T, 16385), False, f"routing {G.NAME[T]} M16385")
    for M in (1, 33):
        check_row(G.row_case("refpoint", 256, T, M), False, f"routing {G.NAME[T]} k512 M{M}")
    check_row(G.row_case("side1_4", 384, T, 16385), True, f"routing {G.NAME[T]} d384 M16385")


def test_measurement_cases_meet_both_bounds_in_f32():
    for T in (F16, BF16):
        for D in (256, 384):
            for seed in range(8):
                check_row(G.rstd_case(D, T, seed), True, f"rstd {G.NAME[T]} d{D} seed {seed}")
                if D == 256:
                    check_row(G.rstd_case(D, T, seed), False, f"rstd {G.NAME[T]} d{D} seed {seed} (row-per-wave)")
        check_enc(G.enc_case(256, 640, T, "narrow", 150, G.GEO, 1, 91, gp=8.0, xscale=2.5), f"silu {G.NAME[T]}")


def test_slot_channels_is_the_packers_permutation():
    from lwdetr_amd import kernels as K
    for D in (256, 384):
        assert slot_channels(D).tolist() == K.vb_kslot_channels(D).tolist()


# ------------------------------------------------------------------------------------------------------------ (2) planted mistakes
ROW_MISTAKES = [("bias of the neighbouring tile", "front", 256), ("gamma / beta exchanged", "back", 256), ("residual rows 8 off", "front", 256),
                ("the stored row includes qpos", "front", 256), ("unrounded hand-over", "back", 256), ("ReLU after rounding with a sign flip", "bbox", 256),
                ("k-halves exchanged", "front", 384), ("k-halves exchanged", "side1_33", 384)]
ENC_MISTAKES = [("a flag indexed by m instead of mm", ("values", "om", "cls")), ("the mask applied before the bias", ("values",)),
                ("gamma / beta exchanged", ("om", "cls")), ("unrounded hand-over", ("om", "cls")), ("the row maximum over all cols", ("cls_max",))]


def leaves(got, tight, worst, T):
    """Does the comparison fail: an element outside the worst-case bound, or more than SHARE of the tensor outside the tight one?"""
    n = got.shape[1]
    cut = lambda ref: tuple(t[:, :n] for t in ref)
    return outside(got, cut(worst), T) > 0 or outside(got, cut(tight), T) > int(G.SHARE * got.numel())


@pytest.mark.parametrize("wrong,name,D", ROW_MISTAKES)
def test_planted_row_mistakes_leave_the_bound(wrong, name, D):
    M = max(m for n, m in G.SPLIT_PROGRAMS if n == name)
    case = G.row_case(name, D, F16, M)
    right, got = emu_row(case, True), emu_row(case, True, wrong)
    assert not any(leaves(right[i], case["tight", True][i], case["worst", True][i], F16) for i in right)
    bad = {i: leaves(got[i], case["tight", True][i], case["worst", True][i], F16) for i in got}
    print(wrong, name, D, bad)
    assert any(bad.values()), f"{wrong}: passes the comparison"


@pytest.mark.parametrize("wrong,names", ENC_MISTAKES)
def test_planted_enc_mistakes_leave_the_bound(wrong, names):
    if wrong != "the row maximum over all cols":
        case = G.enc_case(256, 0, F16, "narrow", 129, G.GEO, 3, 91)
    else:     # one class: the maximum over all 96 columns is max(logit, 0) - wrong wherever the logit is negative
        case = next(c for c in (G.enc_case(256, 0, F16, "narrow", 31, G.GEO, 1, 1, seed=s) for s in range(4)) if bool((emu_enc(c)["cls"][:, 0] < 0).any()))
    got = emu_enc(case, wrong)
    if names == ("cls_max",):
        assert not torch.equal(got["cls_max"], got["cls"][:, :case["ncls"]].max(1).values)
        return
    bad = {n: leaves(got[n], case["tight"][n], case["worst"][n], F16) for n in names}
    print(wrong, bad)
    assert all(bad.values()), f"{wrong}: {bad}"


# ------------------------------------------------------------------------------------------------------------ (3) the ring accounting
class RingModel:
    """One workgroup's ring: DMAs are issued in piece order and land in issue order; a wait names how many of the youngest vector-memory operations may
    still be in flight. Records every violation instead of raising."""

    def __init__(self, nslot, np_):
        self.nslot, self.np = nslot, np_
        self.issued, self.landed = 0, 0              # pieces [0, issued) have a DMA; pieces [0, landed) are covered by a wait
        self.t, self.barrier_t = 0, -1
        self.last_read, self.bad = {}, []
        self.vmseq, self.seq_of, self.slot_piece = 0, {}, {}

    def issue(self, seq=False):
        q = self.issued
        assert q < self.np
        old = q - self.nslot
        if old >= 0 and self.last_read.get(old, -1) >= self.barrier_t:
            self.bad.append(f"piece {q} refills the slot of piece {old} before the barrier that follows its last read")
        self.slot_piece[q % self.nslot] = q
        if seq:
            self.vmseq += 1
            self.seq_of[q % self.nslot] = self.vmseq
        self.issued += 1
        self.t += 1

    def fill(self, first):
        while self.issued < first and self.issued < self.nslot and self.issued < self.np:
            self.issue()

    def wait_all(self):
        self.landed = self.issued

    def wait_count(self, v):
        """s_waitcnt vmcnt(v) when only DMAs count (stores are younger or interleaved: they only make the real wait longer); ch_wait_le: outside 1 .. 31 -> 0."""
        v = v if 1 <= v <= 31 else 0
        self.landed = max(self.landed, self.issued - v)

    def barrier(self):
        self.t += 1
        self.barrier_t = self.t

    def read(self, q, what):
        self.t += 1
        if q > self.np - 1:
            self.bad.append(f"{what}: reads piece {q} beyond piece np - 1 = {self.np - 1}")
            return
        if q >= self.issued:
            self.bad.append(f"{what}: reads piece {q} whose DMA was never issued (issued {self.issued})")
        elif q >= self.landed:
            self.bad.append(f"{what}: reads piece {q} that no wait covers (covered: {self.landed})")
        elif self.slot_piece.get(q % self.nslot) != q:
            self.bad.append(f"{what}: piece {q}'s slot holds piece {self.slot_piece.get(q % self.nslot)}")
        self.last_read[q] = self.t

    # ---- begin_tile (mlp_chain_kernel)
    def begin_tile(self, a, n):
        b = min(a + n + 2, self.np)
        self.wait_count(self.issued - b)
        self.barrier()
        while self.issued < min(a + self.nslot, self.np):
            self.issue()

    # ---- begin_tile_x (enc_chain_kernel): sequence numbers, `need` fetched one tile ahead
    def seq_init(self):
        self.vmseq, self.need, self.lim = 0, 0, self.issued
        self.seq_of = {s: 0 for s in range(self.nslot)}
        self.seq_landed = 0                          # operations with a sequence number <= this have completed

    def flush(self):
        while self.issued < self.lim:
            self.issue(seq=True)

    def stores(self, k):
        self.vmseq += k

    def begin_tile_x(self, a, n, n_next):
        self.flush()
        allowed = self.vmseq - self.need
        allowed = 60 if allowed > 60 else allowed & ~3
        allowed = allowed if allowed >= 4 else 0
        self.seq_landed = max(self.seq_landed, self.vmseq - allowed)
        # pieces covered: every issued piece whose DMA has a sequence number <= seq_landed (in piece order)
        while self.landed < self.issued and self._seq_of_piece(self.landed) <= self.seq_landed:
            self.landed += 1
        self.barrier()
        self.lim = min(a + self.nslot, self.np)
        q = min(a + n + n_next + 1, self.np - 1)
        if self.slot_piece.get(q % self.nslot) != q:
            self.bad.append(f"begin_tile_x({a}, {n}, {n_next}): the wait count of piece {q} is fetched before its DMA was issued "
                            f"(its slot's entry belongs to piece {self.slot_piece.get(q % self.nslot)})")
        self.need = self.seq_of[q % self.nslot]
        self.flush()

    def _seq_of_piece(self, q):
        return self._piece_seq.get(q, 0)

    def track_seq(self):
        """Remember the sequence number of every piece (the kernel keeps them per slot; the model needs them per piece to know what has landed)."""
        self._piece_seq = {}
        orig = self.issue

        def issue(seq=False):
            q = self.issued
            orig(seq)
            self._piece_seq[q] = self.vmseq if seq else 0
        self.issue = issue


def ring_row(D, k_in, stages):
    """mlp_chain_kernel's walk; stages: (kind, n). Returns the violations."""
    PPT, PPT0 = D // 64, k_in // 64
    nts = [(D // 32, PPT0 if i == 0 else PPT) if k == "full" else ((n + 31) // 32, PPT) for i, (k, n) in enumerate(stages)]
    np_ = sum(nt * p for nt, p in nts) + 2
    r = RingModel(32, np_)
    r.fill(PPT0 + 2 + 4)
    r.wait_all()
    r.begin_tile(0, PPT0)
    for p in (0, 1):
        r.read(p, "initial read-ahead")
    pc, first = 0, True
    for si, (nt, ppt) in enumerate(nts):
        for n in range(nt):
            if not first:
                r.begin_tile(pc, ppt)
            first = False
            for f in range(4 * ppt):                 # fragment f is consumed from the read-ahead registers; fragment f + CH_RD is read
                r.read((4 * pc + f + CH_RD) // 4, f"stage {si} tile {n} fragment {f} + {CH_RD}")
            pc += ppt
    assert pc + 2 == np_
    return r.bad


def ring_split(D, stages):
    """mlp_chain_split_kernel's walk (groups of up to 4 tiles, one per wave; D = 384: two k-half steps per group)."""
    PPT = D // 64
    halves = 2 if D == 384 else 1
    PPH, nslot = PPT // halves, 24 if D == 384 else 32
    nts = [D // 32 if k == "full" else (n + 31) // 32 for k, n in stages]
    np_ = sum(nts) * PPT + 2
    r = RingModel(nslot, np_)
    r.fill(nslot)
    r.wait_all()
    pc = 0
    for si, nt in enumerate(nts):
        for g0 in range(0, nt, 4):
            ng = min(4, nt - g0)
            for hf in range(halves):
                b = min(pc + ng * PPH, np_)
                v = r.issued - b
                r.wait_all() if v <= 0 else r.wait_count(v)
                r.barrier()
                while r.issued < min(pc + nslot, np_):
                    r.issue()
                for w in range(ng):
                    for f in range(4 * PPH):
                        r.read((4 * (pc + w * PPH) + f) // 4, f"stage {si} group {g0} half {hf} wave {w} fragment {f}")
                pc += ng * PPH
    assert pc + 2 == np_
    return r.bad


def enc_tile_table(D, k5, nl, cols):
    """One row per tile of enc_chain_kernel, in order: (stage, n = pieces of the tile, n_next = what the kernel passes to begin_tile_x as the next
    tile's pieces, vector stores the wave issues after the tile). Written stage by stage from chain_enc_body.h:
      cv2     (PF only) NTI tiles of PPT5 pieces; tile 0: begin_tile_x(0, PPT5, PPT5), tile n > 0: begin_tile_x(pc, PPT5, n + 1 < NTI ? PPT5 : PPT);
              layernorm_store after the last one: stores(2 NTI)
      values  nl NTI tiles of PPT pieces, begin_tile_x(pc, PPT, PPT) (without cv2 the first one IS the kernel's first tile: begin_tile_x(0, PPT, PPT));
              stores(2) after each
      enc     NTI tiles, begin_tile_x(pc, PPT, PPT); layernorm_store after the last one: stores(2 NTI)
      class   cols / 32 tiles, begin_tile_x(pc, PPT, PPT) - also for the very last tile, which has no successor; stores(2) after each."""
    NTI, PPT, PPT5 = D // 32, D // 64, k5 // 64
    rows = []
    if k5:
        rows += [("cv2", PPT5, PPT5 if n == 0 or n + 1 < NTI else PPT, 2 * NTI if n == NTI - 1 else 0) for n in range(NTI)]
    rows += [("values", PPT, PPT, 2) for _ in range(nl * NTI)]
    rows += [("enc", PPT, PPT, 2 * NTI if n == NTI - 1 else 0) for n in range(NTI)]
    rows += [("class", PPT, PPT, 2) for _ in range(cols // 32)]
    return rows


def ring_enc(D, k5, nl, cols):
    """enc_chain_kernel's walk over enc_tile_table. Returns the violations."""
    PPT, PPT5 = D // 64, k5 // 64
    tiles = enc_tile_table(D, k5, nl, cols)
    np_ = sum(t[1] for t in tiles) + 2
    r = RingModel(32, np_)
    r.track_seq()
    r.fill(2 * (PPT5 if k5 else PPT) + 2)
    r.wait_all()
    r.seq_init()
    pc = 0
    for i, (stage, n, n_next, st) in enumerate(tiles):
        r.begin_tile_x(pc, n, n_next)
        if i == 0:
            for p in (0, 1):
                r.read(p, "initial read-ahead")
        if i + 1 < len(tiles) and n_next != tiles[i + 1][1]:
            r.bad.append(f"{stage} tile {i}: n_next {n_next} is not the next tile's {tiles[i + 1][1]} pieces")
        for f in range(4 * n):
            r.read((4 * pc + f + CH_RD) // 4, f"{stage} tile {i} fragment {f} + {CH_RD}")
        pc += n
        r.stores(st)
    assert pc + 2 == np_
    return r.bad


def test_enc_tile_table_is_the_kernels_stream():
    """The table's pieces add up to lwdetr_enc_chain_pieces_cls, and one written-out instance: D = 256 with cv2, one layer, 96 class columns."""
    from lwdetr_amd import _native
    lib = _native.lib()
    for D, k5 in G.ENC_FORMS:
        for nl in (1, 2, 3, 6):
            for cols, ncls in ((96, 91), (384, 366)):
                assert sum(t[1] for t in enc_tile_table(D, k5, nl, cols)) + 2 == lib.lwdetr_enc_chain_pieces_cls(D, k5, nl, ncls)
    assert enc_tile_table(256, 640, 1, 96) == ([("cv2", 10, 10, 0)] * 7 + [("cv2", 10, 4, 16)] + [("values", 4, 4, 2)] * 8 + [("enc", 4, 4, 0)] * 7
                                               + [("enc", 4, 4, 16)] + [("class", 4, 4, 2)] * 3)


def _kinds(stages):
    return [("full", 0) if st["kind"] == "full" else ("side", st["n"]) for st in stages]


def test_ring_model_on_every_chain_the_gpu_module_launches():
    for D in (256, 384):
        for name, _ in G.SPLIT_PROGRAMS + [("side1_4", 0)]:
            assert ring_split(D, _kinds(G.program(name, D)[0])) == [], (D, name)
    for name in sorted({n for n, _, _ in G.ROW_PROGRAMS} | {"side1_4"}):
        st, k_in, _, _, _ = G.program(name, 256)
        assert ring_row(256, k_in, _kinds(st)) == [], name
    assert ring_split(256, [("full", 0)]) == [] and ring_row(256, 256, [("full", 0)]) == []          # the rstd measurement's chain
    for D, k5 in G.ENC_FORMS:
        for nl in (1, 2, 3, 6):
            for cols in (96, 384):
                assert ring_enc(D, k5, nl, cols) == [], (D, k5, nl, cols)


def test_ring_model_sweep_of_all_programs_up_to_three_stages():
    opts = [("full", 0)] + [("side", n) for n in (1, 32, 33, 96, 576)]
    n = 0
    for nst in (1, 2, 3):
        for prog in itertools.product(opts, repeat=nst):
            prog = list(prog)
            for D in (256, 384):
                assert ring_split(D, prog) == [], (D, prog)
            assert ring_row(256, 256, prog) == [], prog
            if prog[0][0] == "full":
                assert ring_row(256, 512, prog) == [], prog
            n += 1
    assert n == 6 + 36 + 216


def test_ring_model_flags_a_ring_that_is_too_small_and_a_missing_wait():
    """The model is not vacuous: a chain walked with a ring of 8 slots (a tile of 4 pieces + 2 read ahead + the refill window do not fit), a read
    without its wait, and a wait count fetched for a piece that was not issued are all reported."""
    r = RingModel(8, 40)
    r.fill(8)
    r.wait_all()
    r.barrier()
    for q in range(6):
        r.read(q, "tile 0")
    r.begin_tile(4, 4)                               # refills up to piece 11: the slots of pieces 0 .. 3 - fine; then read 10: covered? issued 12, wait leaves 2
    r.read(4, "tile 1")
    r.issue()                                        # piece 12 into the slot of piece 4, which was read after the last barrier
    assert any("before the barrier" in b for b in r.bad)
    r2 = RingModel(32, 40)
    r2.fill(6)
    r2.read(3, "no wait")
    r2.read(7, "not issued")
    r2.read(40, "beyond")
    assert len(r2.bad) == 3 and "no wait covers" in r2.bad[0] and "never issued" in r2.bad[1] and "beyond piece" in r2.bad[2]
    # PF-like tiles of 11 pieces: 11 + 11 + 11 + 1 >= 32, the wait count of the next tile's last piece would be fetched before its DMA
    r3 = RingModel(32, 100)
    r3.track_seq()
    r3.fill(24)
    r3.wait_all()
    r3.seq_init()
    r3.begin_tile_x(0, 11, 11)
    r3.begin_tile_x(11, 11, 11)
    assert any("fetched before its DMA was issued" in b for b in r3.bad)
