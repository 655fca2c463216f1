"""What the compute contexts are made of (csrc/mgx_hip_util.h: the device pick, Owner, DevArray, PinBuf, Mirror) as a stand-alone
program under AddressSanitizer + UBSan with the HIP devices hidden from it, so that every HIP call fails: a create that fails
half way holds nothing, reports its first failure, and can be released and destroyed.  tests/cpp/hip_ctx_driver.cpp has the checks."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "fast-genomic-data-processing_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("no hipcc")
    exe = str(tmp_path_factory.mktemp("hip_ctx") / "driver")
    subprocess.check_call([HIPCC, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer", "-Wall", "-I", CSRC, "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "hip_ctx_driver.cpp"), os.path.join(CSRC, "mgx_common.cpp"), "-o", exe])
    return exe


def test_failure_paths_without_a_device(driver, tmp_path):
    # on a host with GPUs the HSA runtime starts up before it hides them, and keeps 144 bytes of its own: not this project's to free
    supp = tmp_path / "lsan.supp"
    supp.write_text("leak:libhsa-runtime64\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               LSAN_OPTIONS="suppressions=%s:print_suppressions=0" % supp)
    res = subprocess.run([driver], capture_output=True, text=True, env=env, timeout=120)
    if res.returncode == 77:
        pytest.skip("the driver sees a HIP device although they are hidden from it")
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout[-2000:] + res.stderr[-4000:]
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr, res.stderr[-4000:]
