"""Shape of K1m's steady tile loop in the built gfx950 object (CPU only; disassembly, no measurement).

For hamming_mfma_kernel<0,4>, <0,2> and <1,2> the steady loop is the innermost loop that holds exactly
32 * MB MFMAs between its header and its back edge on the fall-through path (conditional branches not
taken).  In that run:
  * no s_nop stands directly in front of a v_mfma or an s_waitcnt, and the run holds at most 6 s_nop
    (hamming_mfma.hip's header names the hazard each remaining one covers);
  * the fall-through path holds at most 5 conditional branches at MB = 4 -- reached: 5 in the thresholded
    instances (one hit-extraction branch per n-block, the > 64-hits test, the flushed-store test, the back
    edge), 1 in the dense one (the back edge) -- and none of them tests `steady` or `t == 0`: the run
    compares no scalar against the tile counter except for the back edge;
  * the kernel uses no scratch and at most 512 registers (descriptor metadata);
  * no register filled by an inline-asm LDS read is touched before its wait (isa_check)."""
import os
import re
import subprocess

import pytest

import isa_check
from vectorragquantization_amd import _native as N

INSTANCES = {"<0,4>": ("hamming_mfma_kernelILi0ELi4EE", 4),
             "<0,2>": ("hamming_mfma_kernelILi0ELi2EE", 2),
             "<1,2>": ("hamming_mfma_kernelILi1ELi2EE", 2)}
MAX_NOPS = 6
MAX_CBRANCH = 5


def is_mfma(x):
    """An MFMA of the tile loop.  llvm-objdump prints the ones whose A operand is a[252:255] as a raw first
    word (`.long 0xd3ae....`: it decodes the f8f6f4 operand eight registers wide, past the file's end, before
    it looks at cbsz) followed by one mis-decoded scalar instruction, which `second_word` names."""
    return x[1].startswith("v_mfma") or (x[1] == ".long" and x[2] and x[2][0].lower().startswith("0xd3ae"))


def second_word(ins, i):
    return i > 0 and ins[i - 1][1] == ".long" and is_mfma(ins[i - 1])


def fallthrough_run(ins, head, back):
    """Instruction indices on the fall-through path from index `head` to the back edge at index `back`:
    conditional branches not taken, unconditional ones followed.  None when the path leaves [head, back]."""
    idx = {a: i for i, (a, *_r) in enumerate(ins)}
    run, i, seen = [], head, set()
    while True:
        if i in seen or i < head or i > back:
            return None
        seen.add(i)
        if not second_word(ins, i):
            run.append(i)
        if i == back:
            return run
        _a, op, _t, _s, tgt = ins[i]
        if op.startswith("s_branch"):
            if tgt not in idx:
                return None
            i = idx[tgt]
        elif op.startswith(("s_endpgm", "s_setpc")):
            return None
        else:
            i += 1


def steady_loop(ins, mb):
    """The innermost loop whose fall-through run holds exactly 32 * mb MFMAs: its run of indices."""
    idx = {a: i for i, (a, *_r) in enumerate(ins)}
    best = None
    for e, (_a, op, _t, _s, tgt) in enumerate(ins):
        if not op.startswith(("s_branch", "s_cbranch")) or tgt not in idx or idx[tgt] > e:
            continue
        run = fallthrough_run(ins, idx[tgt], e)
        if run is None or sum(1 for i in run if is_mfma(ins[i])) != 32 * mb:
            continue
        if best is None or len(run) < len(best):
            best = run
    return best


def loop_counts(ins, run):
    ops = ["v_mfma" if is_mfma(ins[i]) else ins[i][1] for i in run]
    c = {"mfma": 0, "valu": 0, "salu": 0, "ds": 0, "waitcnt": 0, "nop": 0, "cbranch": 0, "branch": 0, "vmem": 0}
    for op in ops:
        if op.startswith("v_mfma"):
            c["mfma"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        elif op == "s_waitcnt":
            c["waitcnt"] += 1
        elif op == "s_nop":
            c["nop"] += 1
        elif op.startswith("s_cbranch"):
            c["cbranch"] += 1
        elif op.startswith("s_branch"):
            c["branch"] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("s_") and op != "s_barrier":
            c["salu"] += 1
    return c


def kernel_notes(co):
    """{kernel symbol: {field: int}} from the code object's amdhsa metadata note."""
    r = subprocess.run([os.path.join(isa_check.LLVM_BIN, "llvm-readelf"), "--notes", co], capture_output=True,
                       text=True, check=True)
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)\s*$", ln)
        if not m:
            continue
        if ln.lstrip().startswith("- ."):  # a new list entry: a kernel record or an argument record
            cur = {}
            out.setdefault("_records", []).append(cur)
        if cur is not None:
            cur[m[1]] = m[2]
    return {r_["name"]: r_ for r_ in out.get("_records", []) if "name" in r_ and "vgpr_count" in r_}


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    N.load()
    obj = os.path.join(N._build.OBJDIR, "hamming_mfma.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(isa_check.LLVM_BIN, "llvm-objdump")):
        pytest.skip("no built object or no ROCm llvm tools")
    wd = str(tmp_path_factory.mktemp("k1m_shape"))
    dis = isa_check.disassemble(obj, wd)
    return {"dis": dis, "funcs": isa_check.parse(dis), "co": os.path.join(wd, "hamming_mfma.o.co")}


def _kernel(funcs, key):
    names = [k for k in funcs if key in k]
    assert len(names) == 1, names
    return names[0]


@pytest.mark.parametrize("inst", sorted(INSTANCES))
def test_steady_loop_has_no_idle_states_in_front_of_mfma(built, inst):
    key, mb = INSTANCES[inst]
    ins = built["funcs"][_kernel(built["funcs"], key)]
    run = steady_loop(ins, mb)
    assert run is not None, "no loop with exactly %d MFMAs on its fall-through path" % (32 * mb)
    ops = ["v_mfma" if is_mfma(ins[i]) else ins[i][1] for i in run]
    c = loop_counts(ins, run)
    print(inst, c)
    bad = [(ins[run[k]][3], ins[run[k + 1]][3]) for k in range(len(run) - 1)
           if ops[k] == "s_nop" and (ops[k + 1].startswith("v_mfma") or ops[k + 1] == "s_waitcnt")]
    assert not bad, bad[:4]
    assert c["nop"] <= MAX_NOPS, c


@pytest.mark.parametrize("inst", sorted(INSTANCES))
def test_steady_loop_has_no_mode_tests(built, inst):
    key, mb = INSTANCES[inst]
    ins = built["funcs"][_kernel(built["funcs"], key)]
    run = steady_loop(ins, mb)
    assert run is not None
    c = loop_counts(ins, run)
    print(inst, c)
    assert c["cbranch"] <= MAX_CBRANCH, [ins[i][3] for i in run if ins[i][1].startswith("s_cbranch")]
    # Neither `steady` (t < nsteady) nor `t == 0` is evaluated in the run.  The tile counter is the scalar the
    # run steps by one (up or down); the only compare that names it is the loop's own exit test (the parent also compared it
    # with nsteady, twice, and with zero).  No scalar bool is selected (s_cselect_b64) or turned into a branch
    # condition (s_and_b64 / s_andn2_b64 vcc, exec, ...): the hit tests branch on a vector compare's vcc.
    text = [ins[i][3] for i in run]
    counters = {m[1] for s in text for m in [re.fullmatch(r"s_add_i32\s+(s\d+),\s*(s\d+),\s*-?1", s)] if m and m[1] == m[2]}
    assert len(counters) == 1, counters
    t_reg = counters.pop()
    t_cmps = [s for s in text if s.startswith("s_cmp") and re.search(r"\b%s\b" % t_reg, s)]
    assert len(t_cmps) == 1, t_cmps
    assert not [s for s in text if s.startswith("s_cselect_b64")]
    assert not [s for s in text if re.match(r"s_andn?2?_b64\s+vcc,\s*exec,", s)]


@pytest.mark.parametrize("inst", sorted(INSTANCES))
def test_descriptor_no_scratch_at_most_512_registers(built, inst):
    key, _mb = INSTANCES[inst]
    notes = kernel_notes(built["co"])
    name = _kernel(notes, key)
    rec = notes[name]
    assert int(rec["private_segment_fixed_size"]) == 0, rec
    assert int(rec["vgpr_count"]) <= 512, rec  # (unified file: this count includes the AGPRs)
    assert int(rec.get("vgpr_spill_count", 0)) == 0 and int(rec.get("sgpr_spill_count", 0)) == 0, rec


def test_no_copies_of_inflight_lds_reads_in_k1m(built):
    keys = [k for k, _ in INSTANCES.values()]
    bad = [v for v in isa_check.copies_of_inflight_lds_reads(built["dis"]) if any(k in v[0] for k in keys)]
    assert not bad, bad[:5]
