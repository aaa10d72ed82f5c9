"""CPU: the weight packer (csrc/weight_pack.h) produces, byte for byte, the buffers the engine uploaded before the packer existed.

tests/native/weight_pack_digest.cpp, built with the ROCm host compiler under AddressSanitizer + UndefinedBehaviorSanitizer, packs every
case below and prints the scalar geometry and one line per device buffer: the plan pointer it fills, its byte length and the FNV-1a-64 of
its bytes (for an f16 GEMM also of the dW / shift0 that calibration keeps).  tests/golden/weight_pack_digests.json holds those lines as
recorded from the engine of the commit BEFORE the packer: its own planners ran with device allocation replaced by host memory and
every upload digested, on the same descriptors and blobs.  The sorted lines must be equal.

Cases: the four topologies x the four dtypes with population BN and fp32 with batch BN; DNA at the segment lengths that switch the
Winograd form (400: F(4,3); 64 and 402: F(2,3); 401: none); each PackSwitches field flipped where it has an effect; and weights with one
planted value per branch of the code (see planted())."""
import json
import os
import subprocess
from collections import OrderedDict

import numpy as np
import pytest

import chiron_amd as ca

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden", "weight_pack_digests.json")
DTYPES = {"fp32": 0, "fp16": 1, "fp32-split": 2, "fp16-w2": 3}
SPECS = {"dna": ca.dna_default_spec, "rna": ca.rna_default_spec, "rna_model2": lambda bn: ca.rna_head_spec("rna_model2", bn),
         "rna_model3": lambda bn: ca.rna_head_spec("rna_model3", bn)}
# the digest program's letters, and the environment switch of the engine each stands for
SWITCHES = {"w": "CHIRON_NO_WINOGRAD", "W": "CHIRON_WINOGRAD_F2", "F": "CHIRON_WINOGRAD_F4", "p": "CHIRON_NO_PWL", "R": "CHIRON_SPLIT_REC32",
            "S": "CHIRON_SPLIT_NO_ROW_SCALE"}


def random_weights(spec, seed):
    """Every tensor of the blob from one RandomState: filters and kernels ~ N(0, 0.1), BN scale and variance in [0.5, 1.5)"""
    rng = np.random.RandomState(seed)
    w = OrderedDict()
    for name, shape in spec.blob_layout().items():
        if name.endswith("_bn/scale") or name.endswith("_bn/pop_var"):
            w[name] = rng.uniform(0.5, 1.5, size=shape).astype(np.float32)
        else:
            w[name] = (0.1 * rng.standard_normal(size=shape)).astype(np.float32)
    return w


def planted(spec, w):
    """One value per branch the packer shows.  Block 1 is the lifted block (its conv2a is a scale / shift per channel)."""
    a, bn = "res_layer1/branch2/conv2a/weights", "res_layer1/branch2/conv2a_bn/"
    w[bn + "pop_mean"][:8] = 0.0
    w[a][0, 0, 0, 0], w[bn + "offset"][0] = 0.0, 0.5          # PWL: a == 0 and b > 0: active from the start, no breakpoint
    w[a][0, 0, 0, 1], w[bn + "offset"][1] = 0.0, -0.5         # a == 0 and b <= 0: never active
    w[bn + "scale"][2] = -1.0                                 # a negative BN scale: a channel that switches OFF going up
    w[a][0, 0, 0, 3], w[bn + "offset"][3] = 1e-30, 0.5        # folded scale 1e-30: a finite breakpoint far outside the signal
    w[a][0, 0, 0, 4], w[bn + "offset"][4] = 1e-30, 1e9        # ... and breakpoints that round to -inf / +inf
    w[a][0, 0, 0, 5], w[bn + "offset"][5] = 1e-30, -1e9
    w["res_layer2/branch2/conv2b/weights"][:, :, :, 5] = 0.0  # an all-zero GEMM row (fp32-split: mx == 0)
    c = "res_layer1/branch2/conv2c"                           # a row of 1e-30 with shift 1e30 (split: the scaled shift overflows, s = 0)
    w[c + "/weights"][:, :, :, 9] = 1e-30
    w[c + "_bn/offset"][9], w[c + "_bn/pop_mean"][9] = 1e30, 0.0
    for name in ("res_layer3/branch2/conv2b/weights", "res_layer2/branch2/conv2a/weights"):
        w[name][0, 0, 7, 11] = 1e-6                           # a half-subnormal lo
        w[name][0, 0, 8, 12] = 7e4                            # above the largest half
    for l in range(spec.rnn_layers):
        k = w[spec.lstm_scope(l, "fw") + "kernel"]
        k[5, 7], k[6, 108], k[-3, 7], k[-2, 208] = 1e-6, 7e4, 1e-6, 7e4   # the same in W_x and W_hh
    return w


def _cases():
    c = OrderedDict()
    for kind in sorted(SPECS):
        L = 400 if kind == "dna" else 500
        for dtype in sorted(DTYPES):
            c["%s-%s-%d" % (kind, dtype, L)] = (kind, "population", dtype, L, "", False)
        c["%s-fp32-batch-%d" % (kind, L)] = (kind, "batch", "fp32", L, "", False)
    for L in (64, 402, 401):
        c["dna-fp32-%d" % L] = ("dna", "population", "fp32", L, "", False)
    for sw, dtype, L in (("w", "fp32", 400), ("W", "fp32", 400), ("F", "fp32", 64), ("p", "fp32", 400), ("R", "fp32-split", 400), ("S", "fp32-split", 400)):
        c["dna-%s-%d-%s" % (dtype, L, SWITCHES[sw])] = ("dna", "population", dtype, L, sw, False)
    for dtype in sorted(DTYPES):
        c["dna-%s-400-planted" % dtype] = ("dna", "population", dtype, 400, "", True)
    c["dna-fp32-split-400-planted-CHIRON_SPLIT_NO_ROW_SCALE"] = ("dna", "population", "fp32-split", 400, "S", True)
    return c


CASES = _cases()


def case_inputs(name):
    """-> (spec, blob, segment_len, dtype number, switch letters)"""
    kind, bn, dtype, L, sw, plant = CASES[name]
    spec = SPECS[kind](bn)
    w = random_weights(spec, 1000 + sorted(SPECS).index(kind))
    return spec, spec.pack(planted(spec, w) if plant else w), L, DTYPES[dtype], sw


def rocm_prefix():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")     # csrc/Makefile's
    return os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))


@pytest.fixture(scope="module")
def digest_exe(tmp_path_factory):
    rocm = rocm_prefix()
    exe = str(tmp_path_factory.mktemp("weight_pack") / "weight_pack_digest")
    cmd = [os.path.join(rocm, "llvm", "bin", "clang++"), "-x", "c++", "-std=c++17", "-O1", "-g", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(HERE, "native", "weight_pack_digest.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return exe


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_holds_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_packed_bytes_equal_what_the_engine_uploaded_before_the_packer(digest_exe, recorded, tmp_path, name):
    spec, blob, L, dtype, sw = case_inputs(name)
    with open(str(tmp_path / "desc"), "wb") as f:
        f.write(bytes(spec.to_c()))
    blob.tofile(str(tmp_path / "blob"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([digest_exe, str(tmp_path / "desc"), str(tmp_path / "blob"), str(L), str(dtype), sw or "-"], capture_output=True, text=True,
                       env=env, timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    lines = sorted(r.stdout.splitlines())
    assert len(lines) > 10
    assert lines == recorded[name]
