"""The pin table (simpleraytracer_amd/csrc/pin_table.h), the host bookkeeping of DeviceScene's pinned
offsets and their summaries, exercised alone: tools/pin_table_check.cpp built as a stand-alone program
under AddressSanitizer and UndefinedBehaviorSanitizer, and run. The table makes no HIP call, so this
needs no GPU."""
from __future__ import annotations

import subprocess
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_pin_table_check_under_sanitizers(tmp_path):
    exe = tmp_path / "pin_table_check"
    build = subprocess.run(
        ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
         f"-I{REPO / 'simpleraytracer_amd' / 'csrc'}", str(REPO / "tools" / "pin_table_check.cpp"), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "pin_table_check: ok"
