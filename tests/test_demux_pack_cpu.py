"""CPU: the host packer of chiron_demux_windows (csrc/demux_pack.h: the four match masks of a pattern, the windows on 8-byte
boundaries).

tests/native/demux_pack_check.cpp, built with the ROCm host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, packs
patterns of every length 1 .. 64 with code 4 among them and windows of 0, 1, 7, 8, 9, 150, 4096 and random lengths into buffers
of exactly the stated size, and checks every mask bit, every record, every copied base and every padding byte."""
import os
import subprocess

from chiron_amd import demux  # noqa: F401  the packer belongs to the demux stage: without it there is nothing to check
from test_weight_pack_cpu import rocm_prefix

HERE = os.path.dirname(os.path.abspath(__file__))


def test_demux_packer_under_sanitizers(tmp_path):
    rocm = rocm_prefix()
    exe = str(tmp_path / "demux_pack_check")
    cmd = [os.path.join(rocm, "llvm", "bin", "clang++"), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(HERE, "native", "demux_pack_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "demux pack OK" in r.stdout
