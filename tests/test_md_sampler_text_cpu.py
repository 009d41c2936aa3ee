"""CPU: the message texts of the seven samplers of the device MD loop (csrc/ta_sampler_text.h) against the literal
strings the library produced before the samplers shared one host-side lifecycle. The GPU tests match on the "off" and
"invalid" texts of some getters; nothing else reaches the no-memory texts of ta_md_init. The header is compiled alone,
with -fsanitize=address,undefined, behind a stand-alone driver (tests/native/sampler_text_driver.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensoralloy_amd", "csrc")

# per sampler, in the canonical order: the getter ta_md_get_x finds it off; finds the data of a failed run; ta_md_init
# finds no device memory for it
EXPECT = [
    "ta_md_get_x: sampling is off (ta_md_set_sampling)",
    "ta_md_get_x: a ta_md_run failed and left the sampled data invalid; call ta_md_set_sampling or ta_md_init again",
    "ta_md_init: no device memory for the rings of ta_md_set_sampling; sampling is off",
    "ta_md_get_x: the pair distributions are off (ta_md_set_rdf)",
    "ta_md_get_x: a ta_md_run failed and left the counts invalid; call ta_md_set_rdf or ta_md_init again",
    "ta_md_init: no device memory for the counts of ta_md_set_rdf; the feature is off",
    "ta_md_get_x: the bond-angle distributions are off (ta_md_set_adf)",
    "ta_md_get_x: a ta_md_run failed and left the counts invalid; call ta_md_set_adf or ta_md_init again",
    "ta_md_init: no device memory for the counts of ta_md_set_adf; the feature is off",
    "ta_md_get_x: the bond-orientational order parameters are off (ta_md_set_order)",
    "ta_md_get_x: a ta_md_run failed and left the counts invalid; call ta_md_set_order or ta_md_init again",
    "ta_md_init: no device memory for the buffers of ta_md_set_order; the feature is off",
    "ta_md_get_x: the cluster analysis is off (ta_md_set_clusters)",
    "ta_md_get_x: a ta_md_run failed and left the data invalid; call ta_md_set_clusters or ta_md_init again",
    "ta_md_init: no device memory for the buffers of ta_md_set_clusters; the feature is off",
    "ta_md_get_x: the common neighbour analysis is off (ta_md_set_cna)",
    "ta_md_get_x: a ta_md_run failed and left the data invalid; call ta_md_set_cna or ta_md_init again",
    "ta_md_init: no device memory for the buffers of ta_md_set_cna; the feature is off",
    "ta_md_get_x: the structure factors are off (ta_md_set_sq)",
    "ta_md_get_x: a ta_md_run failed and left the data invalid; call ta_md_set_sq or ta_md_init again",
    "ta_md_init: no device memory for the buffers of ta_md_set_sq; the feature is off",
]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sampler_text") / "sampler_text_driver")
    src = os.path.join(ROOT, "tests", "native", "sampler_text_driver.cpp")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + CSRC]
    if shutil.which("g++"):
        cmd = ["g++"] + flags + [src, "-o", exe]
    else:  # host-only: no HIP header is involved
        from tensoralloy_amd import _lib
        cmd = [_lib.hipcc_path(), "-x", "c++"] + flags + [src, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-3000:]
    return exe


def test_sampler_texts_are_the_parents(driver):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    p = subprocess.run([driver], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
    assert len(EXPECT) == 21
    assert p.stdout.splitlines() == EXPECT
