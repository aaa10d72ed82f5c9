"""CPU: the host walk of chiron_signal_levels (csrc/signal_pack.h: the checks of a read's base starts and bins, the per-base record
the kernel reads, and the rounding rule the kernel shares).

tests/native/signal_pack_check.cpp, built with the ROCm host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, walks
reads of 0, 1, 63, 64, 65, 257 and random numbers of bases in buffers of exactly the stated size, checks every record, plants each
kind of fault at the last place it can sit, and holds the level to a division-free search on 20,000 random spans."""
import os
import subprocess

from chiron_amd import squiggle  # noqa: F401  the packer belongs to the squiggle stage: without it there is nothing to check
from test_weight_pack_cpu import rocm_prefix

HERE = os.path.dirname(os.path.abspath(__file__))


def test_signal_packer_under_sanitizers(tmp_path):
    rocm = rocm_prefix()
    exe = str(tmp_path / "signal_pack_check")
    cmd = [os.path.join(rocm, "llvm", "bin", "clang++"), "-x", "c++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", os.path.join(HERE, "native", "signal_pack_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "signal pack OK" in r.stdout
