"""Instruction stream of K1m's steady tile in the built gfx950 object (CPU only; disassembly, no measurement).

The single in-order wave per SIMD pays the issue time of every instruction of the steady tile that is not an
MFMA, so the stream is capped per kind at the counts measured after the trim (one counted wait per pair of
k-step groups, one wait at the tile's end, the row popcounts in one DS read, one 64-bit shift per unpack unit;
tools/k1m_census.py, record in profiles/k1m_trim_census.jsonl).  The count before it stands next to each cap; the total of non-MFMA instructions must stay strictly below it."""
import os
import sys

import pytest

import isa_check
import test_k1m_loop_shape as shape
from vectorragquantization_amd import _native as N

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import k1m_census  # noqa: E402

# caps per instance: the measured counts                     (before)
CAPS = {"<0,4>": {"mfma": 128, "valu": 139, "salu": 18,     # 128, 143, 17
                  "ds": 50, "waitcnt": 17, "nop": 4},       # 51, 34, 4
        "<0,2>": {"mfma": 64, "valu": 107, "salu": 18,      # 64, 111, 18
                  "ds": 50, "waitcnt": 17, "nop": 4},       # 51, 34, 4
        "<1,2>": {"mfma": 64, "valu": 166, "salu": 14,      # 64, 170, 14
                  "ds": 48, "waitcnt": 17, "nop": 5}}       # 49, 34, 5
NON_MFMA_BEFORE = {"<0,4>": 257, "<0,2>": 226, "<1,2>": 276}


@pytest.fixture(scope="module")
def funcs(tmp_path_factory):
    N.load()
    obj = os.path.join(N._build.OBJDIR, "hamming_mfma.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(isa_check.LLVM_BIN, "llvm-objdump")):
        pytest.skip("no built object or no ROCm llvm tools")
    return isa_check.parse(isa_check.disassemble(obj, str(tmp_path_factory.mktemp("k1m_trim"))))


@pytest.mark.parametrize("inst", sorted(CAPS))
def test_steady_tile_instruction_counts(funcs, inst):
    key, mb = shape.INSTANCES[inst]
    names = [k for k in funcs if key in k]
    assert len(names) == 1, names
    c = k1m_census.census(funcs[names[0]], mb)
    assert c is not None, "no loop with exactly %d MFMAs on its fall-through path" % (32 * mb)
    print(inst, c)
    over = {k: (c[k], cap) for k, cap in CAPS[inst].items() if c[k] > cap}
    assert not over, over
    assert c["mfma"] == CAPS[inst]["mfma"]
    assert c["non_mfma"] < NON_MFMA_BEFORE[inst], c
