"""The pooled traversal step's stack bookkeeping, without a GPU: tests/native/stack_step_check.cpp restates the branchy transition of
csrc/dev_traversal.h (push_far_lds / pop_lds / SPC_TRAV_POP_ / SPC_STACK_DECODE) and the straight-line one the LDS-only step of
trace_pool runs (TravStack::top_lds / next_flat / SPC_STACK_DECODE_SEL) on a 16-entry column and compares them exhaustively: all
16 hit patterns, sp 0 .. 13, inner, leaf and empty-leaf words as children and as the stack's top.  Built as a program of its own with AddressSanitizer and
UndefinedBehaviorSanitizer and run on the CPU: the column is a heap block of its exact size, and every index is checked against
0 .. 15 besides."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flat_step_is_the_branchy_step(tmp_path):
    exe = str(tmp_path / "stack_step_check")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "native", "stack_step_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok (\d+) transitions", r.stdout)
    assert m, r.stdout + r.stderr
    # 16 patterns x 3 distance orders x 81 child kinds x 14 stack heights x 3 tops x 2 leaf counts
    assert int(m.group(1)) == 16 * 3 * 81 * 14 * 3 * 2


def test_the_restated_operations_are_the_header_s():
    """A drift guard for the restatement: the lines of the straight-line operations that decide indices and the new sp stand in
    csrc/dev_traversal.h as they stand in the native program (modulo the column's accessor)."""
    hdr = open(os.path.join(ROOT, "spcbpt-optix7_amd", "csrc", "dev_traversal.h")).read()
    for line in ("const int p2 = sp + (c3 ? 1 : 0);",
                 "const int p1 = p2 + (c2 ? 1 : 0);",
                 "const uint32_t popped = sp == 0 ? (uint32_t)kTravDone : top;",
                 "sp = miss ? (sp > 0 ? sp - 1 : 0) : p1 + (c1 ? 1 : 0);",
                 "return miss ? popped : r0;",
                 "return column()[(sp > 0 ? sp - 1 : 0) * BLOCK];",
                 "lds[sp * BLOCK] = r3;", "lds[p2 * BLOCK] = r2;", "lds[p1 * BLOCK] = r1;"):
        assert line in hdr, line
