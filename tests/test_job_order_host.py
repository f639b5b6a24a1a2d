"""The connect phase's job list, without a GPU: tests/native/job_order_check.cpp instantiates csrc/job_order.h -- the function the
eye kernel calls -- with a wave replayed lane by lane on the host, and checks over live masks and kind bits of 3 x 64 slots (no job,
all general, all emitter, 64 / 65 / 128 / 129 / 192 jobs, one lane only, a seeded random set) that the list is a permutation of
exactly the live slots, general jobs before emitter jobs, each group in (connection, lane) order.  Built as a program of its own with
AddressSanitizer and UndefinedBehaviorSanitizer and run on the CPU: the list is a heap block of its exact size."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_job_list_is_the_live_slots_by_kind(tmp_path):
    exe = str(tmp_path / "job_order_check")
    b = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                        os.path.join(ROOT, "tests", "native", "job_order_check.cpp")], capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.match(r"ok (\d+) lists", r.stdout)
    assert m, r.stdout + r.stderr
    # 10 counts x packed / scattered x 4 kind patterns; 64 lanes x 7 live sets x 8 kind sets; 4 x 3 boundary cases; 4 000 random
    assert int(m.group(1)) == 10 * 2 * 4 + 64 * 7 * 8 + 4 * 3 + 4000


def test_the_kernel_calls_the_checked_function():
    """The eye kernel builds its list with the header's function and masks the kind bit off where it reads a slot."""
    body = open(os.path.join(ROOT, "spcbpt-optix7_amd", "csrc", "eye_kernel_body.h")).read()
    assert "job_list_by_kind<SPCBPT_CONNECTION_N>(" in body
    assert "& ~kJobKindBit" in body
