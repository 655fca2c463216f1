"""The sortmardup CLI's slice cutters (csrc/cli/slice_cut.cpp: file ranges, pieces of a stream or of inflated text, the
header scan of a piece source) under AddressSanitizer + UBSan, CPU build, no device: the translation unit is compiled with
g++ next to tests/cpp/slice_cut_driver.cpp and nothing else -- it must not need the library, zlib or the SAM parser."""
import os
import subprocess

from conftest import ROOT

CLI = os.path.join(ROOT, "fast-genomic-data-processing_amd", "csrc", "cli")


def test_slice_cutters_under_sanitizers(tmp_path):
    exe = str(tmp_path / "slice_cut_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-I", CLI,
                           os.path.join(ROOT, "tests", "cpp", "slice_cut_driver.cpp"), os.path.join(CLI, "slice_cut.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    res = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "rc 0" in res.stdout
