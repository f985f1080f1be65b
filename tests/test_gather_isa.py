"""The step kernel's neighbour gathers keep a whole group of rows in flight.  Checked in the compiled gfx950 code (hipcc
--cuda-device-only -S, no GPU needed): the headline instantiation qstep_kernel<5, 16, 2, 4, false, true> and the self-test
build's gather-only replay (plan_gather_kernel) are compiled from f2v_kernels.hip.h, and in every innermost loop that
gathers a group -- U = 4 rows of two 16-byte loads per lane -- no `s_waitcnt vmcnt(N)` between the group's loads waits
for one of them.  A load behind a per-slot branch (or one the compiler sinks into the predicated interaction after it)
brings such a wait back: one row in flight per item instead of four.  The plain-launch forms also have to keep the waves per SIMD they were measured
at (FORMS), with nothing spilled."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "--cuda-device-only", "-S", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math",
         "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "force2vec_amd", "csrc")]
STEP = "qstep_kernelILi5ELi16ELi2ELi4ELb0ELb1EE"
REPLAY = "plan_gather_kernelILi16ELi2ELi4ELi1EE"
GROUP_LOADS = 4 * 2  # U rows x NB 16-byte loads per lane

pytestmark = pytest.mark.skipif(not os.access(HIPCC, os.X_OK), reason="hipcc is not available")

# plain-launch forms and the waves per SIMD each keeps (512 VGPRs per SIMD lane, allocated in steps of 8): the headline; the
# quarter forms of D <= 64 (U = 8), which trade a sixth wave for all eight rows in flight; option 6 at a D short of the D = 128
# form's width (e.g. 100), which keeps its sixth wave -- and its one-row gather -- because the trade measured slower there
FORMS = {
    "qstep_kernelILi5ELi16ELi2ELi4ELb0ELb1EE": ("qstep_kernel<5, 16, 2, 4, false, true>", 5),
    "qstep_kernelILi5ELi16ELi2ELi4ELb0ELb0EE": ("qstep_kernel<5, 16, 2, 4, false, false>", 5),
    "qstep_kernelILi6ELi16ELi2ELi4ELb0ELb1EE": ("qstep_kernel<6, 16, 2, 4, false, true>", 5),
    "qstep_kernelILi6ELi16ELi2ELi4ELb0ELb0EE": ("qstep_kernel<6, 16, 2, 4, false, false>", 6),
    "qstep_kernelILi5ELi4ELi1ELi8ELb0ELb1EE": ("qstep_kernel<5, 4, 1, 8, false, true>", 5),
    "qstep_kernelILi5ELi8ELi1ELi8ELb0ELb1EE": ("qstep_kernel<5, 8, 1, 8, false, true>", 5),
    "qstep_kernelILi5ELi16ELi1ELi8ELb0ELb1EE": ("qstep_kernel<5, 16, 1, 8, false, true>", 5),
    "qstep_kernelILi5ELi16ELi1ELi8ELb0ELb0EE": ("qstep_kernel<5, 16, 1, 8, false, false>", 5),
}

TU = """#include "f2v_kernels.hip.h"
""" + "".join("template __global__ void f2v::%s(const f2v::StepArgs);\n" % name for name, _ in FORMS.values()) + """
#ifdef F2V_TEST_HOOKS
template __global__ void f2v::plan_gather_kernel<16, 2, 4, 1>(const float *, float *, const f2v::Item *, uint32_t, const uint32_t *,
                                                               uint32_t, float *);
#endif
"""


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """-> build ("product" / "selftest") -> its compiled code, each compiled once"""
    done = {}

    def get(build):
        if build not in done:
            d = tmp_path_factory.mktemp("isa_" + build)
            src, out = str(d / "gather_isa.hip"), str(d / "gather_isa.s")
            with open(src, "w") as f:
                f.write(TU)
            defs = ["-DF2V_TEST_HOOKS"] if build == "selftest" else []
            subprocess.run([HIPCC] + FLAGS + defs + [src, "-o", out], check=True, cwd=str(d), capture_output=True)
            with open(out) as f:
                done[build] = f.read()
        return done[build]
    return get


def function(text, part):
    """-> (symbol, body) of the one kernel whose mangled name holds `part`."""
    m = re.search(r"^(_Z\S*%s\S*):" % part, text, re.M)
    assert m, "no kernel *%s* in the compiled code" % part
    return m.group(1), text[m.end():text.index(".Lfunc_end", m.end())]


def metadata(text, symbol):
    for entry in re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):]):
        if re.search(r"\.name:\s+%s\s*\n" % re.escape(symbol), entry):
            return {k: int(v) for k, v in re.findall(r"\.(vgpr_count|vgpr_spill_count|private_segment_fixed_size):\s+(\d+)", entry)}
    raise AssertionError("no metadata for " + symbol)


def inner_loops(body):
    """-> {header: [lines of the loop's blocks from its header on, in code order]} for every innermost loop (the compiler's
    own loop comments: `=>This Inner Loop Header`, `in Loop: Header=...`)."""
    blocks, cur = [], None
    for line in body.splitlines():
        m = re.match(r"^(\.LBB(\d+_\d+)|; %bb\.\d+):(.*)$", line)
        if m:
            cur = {"name": "BB" + m.group(2) if m.group(2) else None, "note": m.group(3), "lines": []}
            blocks.append(cur)
        elif cur is not None:
            if not cur["lines"] and re.match(r"^\s*;\s*=>\s*This Inner Loop Header", line):
                cur["note"] += line  # (the header comment may sit on its own line)
            cur["lines"].append(line)
    loops = {}
    for i, b in enumerate(blocks):
        if b["name"] and "Inner Loop Header" in b["note"]:
            lines = list(b["lines"])
            for c in blocks[i + 1:]:
                if ("Header=%s " % b["name"]) not in c["note"] + " ":
                    break
                lines += c["lines"]
            loops[b["name"]] = lines
    return loops


def group_waits(lines):
    """-> the waits between the loop's first and last 16-byte row load of a group that wait for one of the group's own rows:
    a vmcnt(N) after k of them have been issued, N < k.  (Waits for older loads -- the ids of the group, requested a group
    ago -- leave at least the k rows in flight.)"""
    at = [i for i, l in enumerate(lines) if re.search(r"\bglobal_load_dwordx4\b", l)]
    first, last = at[0], at[GROUP_LOADS - 1]
    bad, issued = [], 0
    for l in lines[first:last + 1]:
        if re.search(r"\bglobal_load_dwordx4\b", l):
            issued += 1
        m = re.search(r"s_waitcnt\b.*\bvmcnt\((\d+)\)", l)
        if m and int(m.group(1)) < issued:
            bad.append("%s (after %d of the group's loads)" % (l.strip(), issued))
    return bad


def gather_loops(body):
    return {h: l for h, l in inner_loops(body).items() if sum(1 for x in l if re.search(r"\bglobal_load_dwordx4\b", x)) >= GROUP_LOADS}


@pytest.mark.parametrize("build", ["product", "selftest"])
def test_step_kernel_keeps_a_group_of_rows_in_flight(compiled, build):
    text = compiled(build)
    _, body = function(text, STEP)
    loops = gather_loops(body)
    # the neighbour loop and the negative-sample loop (-bs 1, ns > 8) are both qprocess
    assert len(loops) >= 2, "%s: found %d gather loops in %s" % (build, len(loops), STEP)
    for header, lines in loops.items():
        assert group_waits(lines) == [], "%s: loop %s drains vmcnt between its row loads" % (build, header)


@pytest.mark.parametrize("part", sorted(FORMS))
def test_step_kernel_forms_keep_their_waves_per_simd_without_spills(compiled, part):
    build = "product"  # (the self-test build's kernels carry its hooks: a few more registers, never what ships)
    text = compiled(build)
    symbol, _ = function(text, part)
    md = metadata(text, symbol)
    waves = min(8, 512 // (-(-md["vgpr_count"] // 8) * 8))
    assert waves >= FORMS[part][1], (build, FORMS[part][0], md)
    assert md["vgpr_spill_count"] == 0, (build, FORMS[part][0], md)
    assert md["private_segment_fixed_size"] == 0, (build, FORMS[part][0], md)


def test_gather_replay_keeps_a_group_of_rows_in_flight(compiled):
    _, body = function(compiled("selftest"), REPLAY)  # (plan_gather_kernel exists in the self-test build only)
    loops = gather_loops(body)
    assert loops, "no gather loop in " + REPLAY
    for header, lines in loops.items():
        assert group_waits(lines) == [], "loop %s drains vmcnt between its row loads" % header
