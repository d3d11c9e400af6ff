"""csrc/smst_pcm_tables.h on its own: tests/pcm_tables_layout.cpp, a stand-alone program, checks the layout types against the formulas the
C API wrote out by hand before the header existed.  Built with -fsanitize=address,undefined where the compiler links those runtimes (the
program links them itself, statically, so that nothing depends on the order in which shared libraries load), plain otherwise."""
import os
import subprocess

from conftest import ROOT

SOURCE = os.path.join(ROOT, "tests", "pcm_tables_layout.cpp")
INCLUDES = ["-I", os.path.join(ROOT, "tests", "emu"), "-I", os.path.join(ROOT, "signalsmith-stretch_amd", "csrc")]


def test_pcm_tables_layout(tmp_path):
    exe = str(tmp_path / "pcm_tables_layout")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + INCLUDES + [SOURCE, "-o", exe]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if sanitized.returncode != 0:
        assert "sanitize" in sanitized.stderr or "asan" in sanitized.stderr or "ubsan" in sanitized.stderr, sanitized.stderr   # (only a missing runtime may send us here)
        plain = subprocess.run(base, capture_output=True, text=True)
        assert plain.returncode == 0, plain.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks held" in run.stdout
