"""CPU: the build-time ISA guard (tools/check_isa.py, run by lw-detr_amd/csrc/Makefile on every object) - no packed-f32 VALU
instruction with a non-default op_sel in the product's device code (`v_pk_fma_f32 ... op_sel:[0,1,0]
op_sel_hi:[1,0,0]` returns wrong lanes beside another kernel's MFMA waves on MI355X)."""
import glob
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tools", "check_isa.py")


def test_product_objects_carry_no_crossed_packed_f32():
    objs = sorted(glob.glob(os.path.join(ROOT, "lw-detr_amd", "csrc", "build", "*.o")))
    if not objs:
        pytest.skip("library objects not built here")
    r = subprocess.run([sys.executable, CHECK] + objs, capture_output=True, text=True, env=dict(os.environ, CHECK_ISA_VERBOSE="1"))
    assert r.returncode == 0, r.stderr
    # the check really looked at device code: the GEMM / attention objects hold thousands of (straight) packed-f32 instructions
    counts = {ln.split(":")[1].strip(): int(ln.split(":")[2].split()[0]) for ln in r.stdout.splitlines() if "packed-f32 instructions" in ln}
    assert counts.get("gemm.o", 0) > 1000 and counts.get("msda.o", 1) == 0 and counts.get("topk.o", 1) == 0, counts


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_guard_flags_the_crossed_form(tmp_path):
    src = tmp_path / "bad.hip"
    src.write_text('''#include <hip/hip_runtime.h>
typedef float f2 __attribute__((ext_vector_type(2)));
__global__ void k(float* o, f2 x, f2 b) {
    f2 r;
    asm volatile("v_pk_fma_f32 %0, %1, %2, -0.5 op_sel:[0,1,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(x), "v"(b));
    o[threadIdx.x] = r[0] + r[1];
}
''')
    obj = tmp_path / "bad.o"
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-c", str(src), "-o", str(obj)], stderr=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, CHECK, str(obj)], capture_output=True, text=True)
    assert r.returncode == 1 and "crossed op_sel" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_guard_fails_closed(tmp_path):
    """An object whose device code the guard cannot look at is an ERROR, not a pass (advisor r4): another --offload-arch than the
    one the Makefile passes, or only host objects on the command line."""
    src = tmp_path / "ok.hip"
    src.write_text("#include <hip/hip_runtime.h>\n__global__ void k(float* o) { o[threadIdx.x] = 1.f; }\n")
    obj = tmp_path / "ok.o"
    subprocess.check_call(["hipcc", "--offload-arch=gfx942", "-O3", "-c", str(src), "-o", str(obj)], stderr=subprocess.DEVNULL)
    r = subprocess.run([sys.executable, CHECK, "--arch", "gfx950", str(obj)], capture_output=True, text=True)
    assert r.returncode == 2 and "no code object for" in r.stderr, (r.returncode, r.stderr)
    assert subprocess.run([sys.executable, CHECK, "--arch", "gfx942", str(obj)], capture_output=True, text=True).returncode == 0
    host = tmp_path / "host.o"
    (tmp_path / "host.c").write_text("int f(void) { return 1; }\n")
    subprocess.check_call(["gcc", "-c", str(tmp_path / "host.c"), "-o", str(host)])
    r = subprocess.run([sys.executable, CHECK, str(host)], capture_output=True, text=True)
    assert r.returncode == 2 and "nothing was checked" in r.stderr, (r.returncode, r.stderr)


def test_packed_f16_gelu_kernels_carry_only_straight_forms():
    """Round 5: the block kernel's GELU on packed f16 pairs (vitblock.hip, VB_G16_*; the f16 default) is inline asm written so that the
    op_sel question of section 5d never arises. Checked on the built object: every G16 instantiation holds packed-f16 arithmetic and SDWA
    transcendentals, none of its packed-f16 instructions carries an op_sel / op_sel_hi / neg modifier, every SDWA transcendental selects the
    same word for source and destination and preserves the other half, and a register's two SDWA writes are never adjacent (dst_sel
    forwarding hazard: the hazard recognizer does not look inside inline asm), and every block of them ends on an s_nop."""
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    obj = os.path.join(ROOT, "lw-detr_amd", "csrc", "build", "vitblock.o")
    if not os.path.exists(obj):
        pytest.skip("library objects not built here")
    dis = check_isa.device_disassembly(obj, "gfx950")
    funcs, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", ln)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and "//" in ln:
            cur.append(ln.split("//")[0].strip())
    g16 = {k: v for k, v in funcs.items() if "vitblock_kernel" in k and k.endswith("ELb1EEEvNS_8VbParamsE") and re.search(r"Li[12]ELb1EEEvNS_8VbParamsE$", k)}
    assert len(g16) == 6, sorted(funcs)                     # f16 x {C = 192 x 2 tile forms, C = 384} x {with / without the next block's QKV}
    assert all("IDF16_" in k for k in g16)                  # f16 only: bf16 has no packed arithmetic
    for name, ins in g16.items():
        pk = [i for i in ins if re.match(r"v_pk_(mul|fma|add)_f16\b", i)]
        sd = [i for i in ins if re.match(r"v_(exp|rcp)_f16_sdwa\b", i)]
        assert len(pk) >= 64 and len(sd) >= 64 and len(sd) % 8 == 0, (name, len(pk), len(sd))
        assert not [i for i in pk if "op_sel" in i or "neg_" in i], name
        for i in sd:
            w = re.findall(r"(dst_sel|src0_sel):WORD_([01])", i)
            assert len(w) == 2 and w[0][1] == w[1][1] and "dst_unused:UNUSED_PRESERVE" in i, (name, i)
        for a, b in zip(ins, ins[1:]):
            if a.startswith(("v_exp_f16_sdwa", "v_rcp_f16_sdwa")) and b.startswith(("v_exp_f16_sdwa", "v_rcp_f16_sdwa")):
                assert a.split()[1] != b.split()[1], (name, a, b)          # same destination register back to back
        # round 6 (advisor r5): what follows a block's LAST SDWA write is the compiler's choice and may read its destination - the block
        # therefore ends on a wait state of its own: every run of SDWA transcendentals is followed by an s_nop, never directly by a reader
        for a, b in zip(ins, ins[1:]):
            if a.startswith(("v_exp_f16_sdwa", "v_rcp_f16_sdwa")) and not b.startswith(("v_exp_f16_sdwa", "v_rcp_f16_sdwa")):
                assert b.startswith("s_nop"), (name, a, b)
    # the kernels that existed before do not carry the packed-f16 forms (own instantiations: profiles/r5g_* is why)
    old = {k: v for k, v in funcs.items() if "vitblock_kernel" in k and k not in g16}
    assert len(old) == 12 and not any(re.match(r"v_(exp|rcp)_f16_sdwa\b", i) for v in old.values() for i in v)


def _device_functions(obj):
    import re
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    dis = check_isa.device_disassembly(obj, "gfx950")
    funcs, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", ln)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and "//" in ln:
            cur.append(ln.split("//")[0].strip())
    return funcs


def test_weight_ring_barriers_are_preceded_by_an_lds_read_drain():
    """Round 6 (profiles/r6e_*): the barrier at a weight-ring boundary releases LDS slots to the DMA issued right behind it, so every fragment
    read of those slots must have RETURNED when a wave signals. The source order (consuming MFMAs, then the boundary) does not guarantee that -
    instruction selection may sink the MFMAs and their lgkmcnt waits below the barrier; one such build failed parity in 3 of 6 runs. The
    kernels of vitblock.hip therefore carry `s_waitcnt lgkmcnt(0)` directly in front of every s_barrier, the exact-form ring of chain.hip
    `s_waitcnt lgkmcnt(8)` (all but the read-ahead into the coming tile). Checked on the built objects."""
    import re
    base = os.path.join(ROOT, "lw-detr_amd", "csrc", "build")
    if not os.path.exists(os.path.join(base, "vitblock.o")):
        pytest.skip("library objects not built here")
    funcs = _device_functions(os.path.join(base, "vitblock.o"))
    ring = {k: v for k, v in funcs.items() if re.search(r"vitblock_kernel|vit_qkv_kernel|vit_stem_kernel", k)}
    assert len(ring) >= 18 + 4, sorted(funcs)
    for name, ins in ring.items():
        bars = [i for i, x in enumerate(ins) if x == "s_barrier"]
        assert len(bars) >= 2, (name, len(bars))      # (loops: a static barrier runs many times)
        for b in bars:
            # walking back from the barrier, the drain comes before any LDS read (arithmetic may sit in between: the compiler moves what has
            # no side effect; ds_bpermute / ds_swizzle do not touch LDS memory)
            j = b - 1
            while j >= 0 and not re.search(r"^s_waitcnt .*lgkmcnt\(0\)|^s_waitcnt lgkmcnt\(0\)", ins[j]):
                assert not re.match(r"ds_read|ds_load", ins[j]), (name, b, j, ins[j])
                j -= 1
            assert j >= 0, (name, b)
    funcs = _device_functions(os.path.join(base, "chain.o"))
    enc = {k: v for k, v in funcs.items() if "enc_chain_kernel" in k}
    assert enc, sorted(funcs)
    for name, ins in enc.items():
        bars = [i for i, x in enumerate(ins) if x == "s_barrier"]
        assert bars, name
        for b in bars:
            back = ins[max(0, b - 8):b]
            m = [re.fullmatch(r"s_waitcnt (?:vmcnt\(\d+\) )?lgkmcnt\((\d+)\)", x) for x in back]
            assert any(x and int(x.group(1)) <= 8 for x in m), (name, b, back)


def test_no_lds_read_is_outstanding_at_any_barrier_of_the_library():
    """The same invariant over EVERY kernel of the product library, by counting: walking back from each s_barrier to the closest `s_waitcnt
    ... lgkmcnt(N)` of its block, N plus the LDS reads issued in between = the reads that can still be in flight when the wave signals.
    0 everywhere (a barrier in these kernels hands LDS data or LDS slots to somebody else), except the exact-form ring of the row-chain
    kernels, whose read-ahead of 8 fragments into the coming tile is in flight by design (chain.hip: CH_RD)."""
    import re
    base = os.path.join(ROOT, "lw-detr_amd", "csrc", "build")
    objs = sorted(glob.glob(os.path.join(base, "*.o")))
    if not objs:
        pytest.skip("library objects not built here")
    seen = 0
    for obj in objs:
        for name, ins in _device_functions(obj).items():
            for b in [i for i, x in enumerate(ins) if x == "s_barrier"]:
                j, reads, n = b - 1, 0, None
                while j >= 0:
                    x = ins[j]
                    m = re.search(r"lgkmcnt\((\d+)\)", x)
                    if x.startswith("s_waitcnt") and m:
                        n = int(m.group(1))
                        break
                    if re.match(r"ds_read|ds_load", x):
                        reads += 1
                    if x.startswith(("s_cbranch", "s_branch", "s_endpgm")):
                        break                                  # top of the block: what came before is another path's business
                    j -= 1
                seen += 1
                allowed = 8 if "enc_chain_kernel" in name else 0
                assert reads + (n or 0) <= allowed, (os.path.basename(obj), name, b, reads, n)
    assert seen > 500, seen


# ---- gemm_pt.hip: the `s_waitcnt vmcnt(16)` shortcut of a tile's first k-step -----------------------------------------------------------
# vmcnt retires in order: waiting for at most 16 outstanding vector-memory operations means "every ring piece has landed" only while the
# previous tile's epilogue issued its stores AFTER the ring's newest global_load_lds and no flat_* operation (which may retire out of order,
# MI355X_MICROARCH vmcnt section) sits in between. The check walks the control-flow graph of the built kernel BACKWARD from each shortcut
# wait (the vmcnt(16) that the stage barrier follows; the compiler's own vmcnt(16) inside the epilogue are not it) until a global_load_lds
# ends the path, and requires: no flat_* on any such path; on every path that ends at a ring piece issued inside the tile loop (a strongly
# connected component), an epilogue store; paths that end outside every cycle start at the prologue (first tile: `stores_behind` is still
# false there, the vmcnt(0) branch runs). What the walk cannot count is the 16: the epilogue stores in `#pragma unroll 1` loops and under
# run-time conditions (a ragged tile stores fewer rows and leaves `stores_behind` false; s_cbranch_execz skips, not followed here, are taken
# only with no lane active), so a static path holds as few as one store instruction; that part rests on the source (`stores_behind = ma == m0`, full tiles only), which the test reads as well.
def _cfg(lines):
    """Instructions of one disassembled function -> (addresses, mnemonics, successor lists). Fails closed on a jump it cannot resolve."""
    import re
    addr, mn, text, tgt = [], [], [], []
    for ln in lines:
        m = re.match(r"\s*(\S+)(.*?)//\s*([0-9A-Fa-f]+):[^<]*(?:<\w+\+0x([0-9a-f]+)>)?", ln)
        if not m:
            continue
        mn.append(m.group(1)); text.append(m.group(1) + m.group(2)); addr.append(int(m.group(3), 16))
        tgt.append(int(m.group(4), 16) if m.group(4) else None)
    base = addr[0]
    at = {a: i for i, a in enumerate(addr)}
    succ = []
    for i, op in enumerate(mn):
        nxt = [i + 1] if i + 1 < len(mn) else []
        if op == "s_endpgm":
            succ.append([])
        elif op == "s_branch":
            succ.append([at[base + tgt[i]]])
        elif op.startswith("s_cbranch"):
            succ.append([at[base + tgt[i]]] + nxt)
        elif op == "s_setpc_b64":
            # long jump: s_getpc_b64 s[a:b]; s_add_u32 sa, sa, lit; s_addc_u32 sb, sb, hi; s_setpc_b64 s[a:b]
            j = i - 1
            while j >= 0 and mn[j] != "s_getpc_b64":
                j -= 1
            assert i - j <= 4 and j >= 0, f"unresolved s_setpc_b64 at {addr[i]:#x}: {text[i]}"
            lo = re.search(r"s_add_u32 \w+, \w+, (0x[0-9a-f]+|-?\d+)", " ".join(text[j:i]))
            hi = re.search(r"s_addc_u32 \w+, \w+, (0x[0-9a-f]+|-?\d+)", " ".join(text[j:i]))
            assert lo and hi, f"unresolved s_setpc_b64 at {addr[i]:#x}"
            off = (int(lo.group(1), 0) & 0xffffffff) | ((int(hi.group(1), 0) & 0xffffffff) << 32)
            off = off - (1 << 64) if off >> 63 else off
            succ.append([at[addr[j] + 4 + off]])
        else:
            succ.append(nxt)
    return addr, mn, succ


def _in_cycle(succ):
    """Nodes that lie on a cycle (iterative Tarjan)."""
    n = len(succ)
    index, low, on, stack, out = [-1] * n, [0] * n, [False] * n, [], [False] * n
    counter = 0
    for root in range(n):
        if index[root] >= 0:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                index[v] = low[v] = counter; counter += 1
                stack.append(v); on[v] = True
            if k < len(succ[v]):
                work.append((v, k + 1))
                w = succ[v][k]
                if index[w] < 0:
                    work.append((w, 0))
                elif on[w]:
                    low[v] = min(low[v], index[w])
                continue
            for w in succ[v]:
                if on[w] and index[w] > index[v]:
                    low[v] = min(low[v], low[w])
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop(); on[w] = False; comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    for w in comp:
                        out[w] = True
    return out


def shortcut_waits(lines):
    """For every shortcut `s_waitcnt vmcnt(16)` of one function: (address, fewest stores on a backward path to a ring piece issued inside the
    tile loop, flat_* seen on any backward path, number of paths that end at a ring piece outside every cycle, fewest stores on those)."""
    import re
    from collections import deque
    addr, mn, succ = _cfg(lines)
    txt = [ln.split("//")[0].strip() for ln in lines if re.search(r"//\s*[0-9A-Fa-f]+:", ln)]
    assert len(txt) == len(mn)
    pred = [[] for _ in mn]
    for i, s_ in enumerate(succ):
        for k, j in enumerate(s_):
            if mn[i] == "s_cbranch_execz" and k == 0:
                continue        # taken only when no lane is active: every lane of a full tile's epilogue owns outputs
            pred[j].append(i)
    cyc = _in_cycle(succ)
    sites = []
    for i, t in enumerate(txt):
        if t == "s_waitcnt vmcnt(16)":
            j = i + 1
            while j < len(txt) - 1 and not txt[j].startswith(("s_barrier", "s_waitcnt", "global_", "buffer_", "flat_", "ds_")):
                j += 1
            if txt[j] == "s_barrier":
                sites.append(i)
    res = []
    for w in sites:
        dist = {w: 0}
        dq = deque([w])
        loop_min, flat, pro, pro_min = None, False, 0, None
        while dq:
            v = dq.popleft()
            for p in pred[v]:
                d = dist[v] + (1 if mn[p].startswith("global_store") else 0)
                if p in dist and dist[p] <= d:
                    continue
                dist[p] = d
                if mn[p].startswith("global_load_lds"):           # the ring's newest piece on this path: the path ends here
                    if cyc[p]:
                        loop_min = d if loop_min is None else min(loop_min, d)
                    else:
                        pro, pro_min = pro + 1, d if pro_min is None else min(pro_min, d)
                    continue
                if mn[p].startswith("flat_"):
                    flat = True
                if d > dist[v]:
                    dq.append(p)
                else:
                    dq.appendleft(p)
        res.append((addr[w], loop_min, flat, pro, pro_min))
    return res


def _pt_functions(dis):
    import re
    funcs, cur = {}, None
    for ln in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", ln)
        if m:
            cur = funcs.setdefault(m.group(1), []) if "gemm_pt_kernel" in m.group(1) else None
        elif cur is not None and "//" in ln:
            cur.append(ln)
    return funcs


def _check_pt_vmcnt16(dis):
    funcs = _pt_functions(dis)
    assert len(funcs) == 2, sorted(funcs)                   # f16 and bf16
    for name, lines in funcs.items():
        sites = shortcut_waits(lines)
        assert len(sites) == 2, (name, "expected one shortcut wait per operand order (ROW / COL k-loop)", sites)
        for a, loop_min, flat, pro, pro_min in sites:
            assert not flat, (name, hex(a), "a flat_* operation between the ring's newest piece and vmcnt(16)")
            assert loop_min is not None, (name, hex(a), "no path from a ring piece inside the tile loop")
            assert loop_min >= 1, (name, hex(a), "a loop path with no epilogue store behind the ring's newest piece")
            assert pro >= 1 and pro_min == 0, (name, hex(a), "the first-tile (prologue) paths are not where they were")


def test_pt_vmcnt16_shortcut_paths():
    src = open(os.path.join(ROOT, "lw-detr_amd", "csrc", "gemm_pt.hip")).read()
    # the run-time half of the argument: the shortcut is taken only behind a full tile's epilogue (>= 16 stores per wave), never on the first tile
    assert "bool stores_behind = false;" in src and "stores_behind = ma == m0;" in src
    assert 'if (FIRST && stores_behind) asm volatile("s_waitcnt vmcnt(16)"' in src
    _check_pt_vmcnt16(_pt_disassembly())


def _pt_disassembly():
    obj = os.path.join(ROOT, "lw-detr_amd", "csrc", "build", "gemm_pt.o")
    if not os.path.exists(obj):
        pytest.skip("library objects not built here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    return check_isa.device_disassembly(obj, "gfx950")


def test_pt_vmcnt16_guard_flags_hand_edited_disassembly():
    """The same check on edited copies of the disassembly (every edit keeps the instruction addresses): the epilogue stores renamed to an
    opcode that is not a store, and a flat load in front of a shortcut wait - each one is refused; the unedited text passes."""
    import re
    dis = _pt_disassembly()
    _check_pt_vmcnt16(dis)
    with pytest.raises(AssertionError, match="no epilogue store"):
        _check_pt_vmcnt16(re.sub(r"\tglobal_store_\w+ ", "\tv_nop ", dis))
    ls = dis.splitlines()
    i16 = next(i for i, ln in enumerate(ls) if ln.startswith("\ts_waitcnt vmcnt(16)") and
               next(x for x in ls[i + 1:] if x.startswith("\ts_")).startswith(("\ts_barrier", "\ts_ashr", "\ts_mov", "\ts_add")))
    j = i16 - 1
    while ls[j].split()[0].startswith(("s_cbranch", "s_branch", "s_setpc", "s_getpc", "s_add", "s_endpgm", "s_waitcnt")):
        j -= 1
    edited = ls[:]
    edited[j] = re.sub(r"^\t\S+[^/]*", "\tflat_load_dword v0, v[0:1] ", edited[j])
    with pytest.raises(AssertionError, match="flat_"):
        _check_pt_vmcnt16("\n".join(edited))
