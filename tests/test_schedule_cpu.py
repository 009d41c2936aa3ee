"""CPU: the sample schedule of the device MD loop (csrc/ta_schedule.h, `ta::SampleSchedule`), which the
correlations (`ta_md_set_sampling`) and the pair distributions (`ta_md_set_rdf`) each keep, against brute-force
enumeration in Python. The header is compiled alone, with -fsanitize=address,undefined, behind a stand-alone driver
(tests/native/schedule_driver.cpp)."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensoralloy_amd", "csrc")

EVERY = (1, 2, 3, 7)
START = (0, 1, 6, 7)
TOTAL = 40


def cuts():
    """Every way of cutting TOTAL steps into at most 3 runs, zero-length runs included."""
    out = [(TOTAL,)]
    out += [(a, TOTAL - a) for a in range(TOTAL + 1)]
    out += [(a, b, TOTAL - a - b) for a in range(TOTAL + 1) for b in range(TOTAL + 1 - a)]
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("schedule") / "schedule_driver")
    src = os.path.join(ROOT, "tests", "native", "schedule_driver.cpp")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC]
    if shutil.which("g++"):
        cmd = ["g++"] + flags + [src, "-o", exe]
    else:  # host-only: no HIP header is involved
        from tensoralloy_amd import _lib
        cmd = [_lib.hipcc_path(), "-x", "c++"] + flags + [src, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    return exe


def test_schedule_against_enumeration(driver):
    cases = [(e, s, c) for e, s, c in itertools.product(EVERY, START, cuts())]
    stdin = "".join(f"{e} {s} {len(c)} " + " ".join(map(str, c)) + "\n" for e, s, c in cases)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([driver], input=stdin, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
    lines = iter(p.stdout.splitlines())

    def pairs(line, tag):
        w = line.split()
        assert w[0] == tag, line
        v = list(map(int, w[1:]))
        return list(zip(v[0::2], v[1::2]))

    for every, start, runs in cases:
        assert next(lines) == "C"
        origin = -(-start // every) * every  # the first multiple of `every` at or behind the start
        sampled = []
        step = start
        for n in runs:
            first = pairs(next(lines), "S")
            replay = pairs(next(lines), "R")
            # a launch that is enqueued again after a list rebuild samples what it sampled, under the same index
            assert replay == first, (every, start, runs)
            assert all(step <= t <= step + n for t, _ in first), (every, start, runs, first)
            sampled += first
            step += n
            last, taken = map(int, next(lines).split()[1:])
            reached = [t for t in range(origin, step + 1, every)]
            assert last == (reached[-1] if reached else -1), (every, start, runs, step, last)
            assert taken == len(reached), (every, start, runs, step, taken)
        # every multiple of `every` from the origin to the last step exactly once, numbered from 0 in order
        expect = [(t, i) for i, t in enumerate(range(origin, start + TOTAL + 1, every))]
        assert sampled == expect, (every, start, runs, sampled)
    assert next(lines, None) is None
