"""CPU: the three bf16 planes of the fp32 LSTM projection weights (csrc/weight_pack.h: split_bf16x3, bf16x3_planes).

tests/native/bf16x3_planes_check.cpp, built with the ROCm host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, runs the
plane builder on +-0, 1e-6, 7e4, 1e30, 1e-30, FLT_MAX, FLT_MIN, subnormals, a value with all 24 significand bits set and N x K random
weights, for K = 256 and for K = 200 in rows of 224, and checks: hi + mid + lo == w in double (within 2^-133 where the weight's lowest
bit lies below that), finite parts, the image read back through the DMA / fragment geometry of gemm_proj_bf16x3_kernel restated in the
program, zeros in the padding channels, and that the index function fills the image exactly once."""
import os
import subprocess

from test_weight_pack_cpu import rocm_prefix

HERE = os.path.dirname(os.path.abspath(__file__))


def test_bf16x3_planes_are_exact_and_lie_where_the_kernel_reads_them(tmp_path):
    rocm = rocm_prefix()
    exe = str(tmp_path / "bf16x3_planes_check")
    cmd = [os.path.join(rocm, "llvm", "bin", "clang++"), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "native", "bf16x3_planes_check.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "bf16x3 planes OK" in r.stdout
