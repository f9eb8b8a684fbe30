"""The lane fan's host-only half (grid2op_amd/csrc/gridpf_lane_fan.hpp): tests/native/lane_fan_main.cpp, a stand-alone program with its
own main, built with plain g++ and the address and undefined-behaviour sanitizers -- the split's index arithmetic, and a fetched
moved-lane list that comes out in lane order or is refused whole."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


def test_lane_fan_host_half_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this host")
    exe = tmp_path / "lane_fan"
    cmd = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "native", "lane_fan_main.cpp"), "-o", str(exe)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("ok:") and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-2000:])
