"""
The library's environment switches (csrc/ta_options.{h,cpp}): `options_from_env` is the one place that reads
them, once per handle in ta_create. Its parsing rules, through a small driver (tests/native/options_print.cpp)
that feeds it a fake environment, and that no other file of csrc/ looks at the environment.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensoralloy_amd", "csrc")

SET_AT_ALL = ["TA_NO_JOBS", "TA_FULL_RECORDS", "TA_NO_OWN_SUMS", "TA_NO_LIST_FILTER", "TA_FILTER_REV_KERNEL",
              "TA_FORCE_V1", "TA_NO_ETA_CHAIN", "TA_STAGED_COPY_DMA", "TA_MLP_TILE_KERNEL", "TA_MLP_WAVE_KERNEL",
              "TA_MLP_QUAD_KERNEL", "TA_MLP_DA_GLOBAL", "TA_EAM_NN_GENERIC", "TA_DEBUG_NO_TRIPLES"]
FIRST_IS_1 = ["TA_HOST_NL", "TA_NL_TWO_PASS", "TA_NL_COPY_STARTS", "TA_SYNC_BLOCKING"]
NUMBERS = {"TA_FWD_WPE": 0, "TA_BWD_WPE": 0, "TA_GATHER_W": 0, "TA_COPY_WG_PER_CU": 8, "TA_COPY_MODE": -1}


def field(var):
    return var[3:].lower()


DEFAULTS = dict({field(v): 0 for v in SET_AT_ALL + FIRST_IS_1}, **{field(v): d for v, d in NUMBERS.items()},
                eam_nn_tables=1, debug_skip=-1, stagger_fwd=0, stagger_bwd=0, phase_stamps_out="")


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    from tensoralloy_amd import _lib
    exe = str(tmp_path_factory.mktemp("options") / "options_print")
    cmd = [_lib.hipcc_path(), "-x", "c++", "-std=c++17", "-I" + CSRC, os.path.join(CSRC, "ta_options.cpp"),
           os.path.join(ROOT, "tests", "native", "options_print.cpp"), "-o", exe]
    try:
        built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    except FileNotFoundError:
        pytest.skip("no host compiler")
    assert built.returncode == 0, built.stderr[-3000:]

    def run(**env):
        p = subprocess.run([exe] + [f"{k}={v}" for k, v in env.items()], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0, p.stderr[-3000:]
        out = dict(line.split(" ", 1) for line in p.stdout.splitlines())
        return {k: v if k == "phase_stamps_out" else int(v) for k, v in out.items()}

    return run


def changed(got):
    return {k: v for k, v in got.items() if v != DEFAULTS[k]}


def test_empty_environment_gives_the_defaults(parse):
    assert parse() == DEFAULTS
    assert parse(TA_UNRELATED="1", TA_NO_JOBS_X="1", XTA_NO_JOBS="1") == DEFAULTS


def test_each_variable_switches_its_field_alone(parse):
    for var in SET_AT_ALL:       # set at all: any value, "0" and the empty string included
        for value in ("1", "0", ""):
            assert changed(parse(**{var: value})) == {field(var): 1}, (var, value)
    for var in FIRST_IS_1:       # first character '1'
        assert changed(parse(**{var: "1"})) == {field(var): 1}, var
        assert changed(parse(**{var: "1x"})) == {field(var): 1}, var
        for value in ("0", "", "yes", "01"):
            assert changed(parse(**{var: value})) == {}, (var, value)
    for value in ("0", "0ff"):   # first character '0' switches off
        assert changed(parse(TA_EAM_NN_TABLES=value)) == {"eam_nn_tables": 0}
    for value in ("1", "", "off"):
        assert changed(parse(TA_EAM_NN_TABLES=value)) == {}
    for var, default in NUMBERS.items():   # atoi
        for value, want in (("5", 5), ("-3", -3), ("16", 16), ("2x", 2), ("x", 0), ("", 0)):
            assert changed(parse(**{var: value})) == ({field(var): want} if want != default else {}), (var, value)
    assert changed(parse(TA_PHASE_STAMPS_OUT="/tmp/stamps.txt")) == {"phase_stamps_out": "/tmp/stamps.txt"}


def test_near_misses_of_the_rules(parse):
    assert parse(TA_HOST_NL="0")["host_nl"] == 0             # the host builder stays off
    assert parse(TA_EAM_NN_TABLES="1")["eam_nn_tables"] == 1   # tables stay on
    assert parse(TA_NO_JOBS="0")["no_jobs"] == 1             # set at all: jobs off
    assert parse(TA_GATHER_W="7")["gather_w"] == 7           # stored as given; the launcher takes 16 or 32 only


def test_probe_switches(parse):
    """Parsed like the rest; only a -DTA_PROBE_SWITCHES build of the library looks at them."""
    assert changed(parse(TA_DEBUG_SKIP="5")) == {"debug_skip": 5}
    assert changed(parse(TA_DEBUG_SKIP="0")) == {"debug_skip": 0}
    assert changed(parse(TA_DEBUG_SKIP="133")) == {"debug_skip": 133 & 127}
    assert changed(parse(TA_STAGGER_FWD="4")) == {"stagger_fwd": (4 << 8) | (3 << 16)}
    assert changed(parse(TA_STAGGER_BWD="300,40")) == {"stagger_bwd": ((300 & 0xff) << 8) | ((40 & 31) << 16)}
    assert changed(parse(TA_STAGGER_FWD="x")) == {}


def test_several_variables_at_once(parse):
    got = parse(TA_MLP_QUAD_KERNEL="1", TA_HOST_NL="1", TA_NO_JOBS="1", TA_BWD_WPE="6")
    assert changed(got) == {"mlp_quad_kernel": 1, "host_nl": 1, "no_jobs": 1, "bwd_wpe": 6}


def test_only_ta_options_reads_the_environment():
    """Over the text of csrc/: `getenv` occurs in ta_options.cpp and nowhere else, and ta_options.{h,cpp}
    include nothing of HIP."""
    hits = []
    for name in sorted(os.listdir(CSRC)):
        path = os.path.join(CSRC, name)
        if os.path.isfile(path):
            with open(path, encoding="utf-8", errors="replace") as fp:
                text = fp.read()
            if "getenv" in text:
                hits.append(name)
            if name.startswith("ta_options."):
                assert "#include <hip" not in text and "ta_device.h" not in text, name
    assert hits == ["ta_options.cpp"]
