"""What one trip of the headline step kernel's neighbour loop costs in issue slots.  Checked in the compiled gfx950 code (hipcc
--cuda-device-only -S, no GPU needed; the translation unit and flags of test_gather_isa.py): in qstep_kernel<5, 16, 2, 4, false, true>
the neighbour gather loop -- the first, in code order, of the innermost loops that hold a group's eight 16-byte row loads; the
other is the sample walk of -bs 1 / ns > 8 -- covers 4 gathered rows for each of a wavefront's 4 items.  Counted per trip: the
vector-ALU instructions plus the `s_nop`s (every one is an issue slot of the SIMD), and the fp64 instructions among them.

Before a group's interactions were written out for the ISA the loop compiled to 384 slots (324 VALU + 60 s_nop), 56 of them fp64: the
coefficient -2 / (1 + a) evaluated once per row on all 16 lanes of an item, 52 register moves to pair the two blocks'
squared differences and to copy Y at every predicated interaction, and a move in front of every cross-lane add.  Now the four
rows' coefficients are one fp64 evaluation (lane t takes row t & 3's `a`), the differences and squares are packed in load
order, and the cross-lane adds take their DPP operand directly.

The bounds: at most three quarters of the slots and at most half of the fp64 instructions the loop had before (288, 28), and
never more than what the change compiles to plus about 5 % for compiler noise."""
import os
import re

import pytest

from test_gather_isa import HIPCC, STEP, compiled, gather_loops, function  # noqa: F401  (compiled: the module's fixture)

pytestmark = pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")

PARENT_SLOTS, PARENT_F64 = 384, 56
PINNED_SLOTS, PINNED_F64 = 278, 14  # what the loop compiles to today (240 VALU + 38 s_nop)


def loop_counts(lines):
    """-> (VALU instructions, s_nops, fp64 instructions) of a loop's lines"""
    ops = [m.group(1) for m in (re.match(r"^\s+([a-z][a-z0-9_]+)\b", l) for l in lines) if m]
    valu = [o for o in ops if o.startswith("v_")]
    return len(valu), sum(1 for o in ops if o == "s_nop"), sum(1 for o in valu if "f64" in o)


def neighbour_loop(text):
    _, body = function(text, STEP)
    loops = gather_loops(body)
    assert len(loops) >= 2, "found %d gather loops in %s" % (len(loops), STEP)
    return next(iter(loops.values()))  # (dicts keep code order)


def test_neighbour_loop_issue_slots(compiled):
    valu, nops, f64 = loop_counts(neighbour_loop(compiled("product")))
    print("neighbour loop of %s: %d VALU + %d s_nop = %d issue slots, %d fp64" % (STEP, valu, nops, valu + nops, f64))
    assert valu + nops <= min(round(PINNED_SLOTS * 1.05), PARENT_SLOTS * 3 // 4), (valu, nops)
    assert f64 <= min(round(PINNED_F64 * 1.05), PARENT_F64 // 2), f64
