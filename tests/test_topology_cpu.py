"""CPU: the topology table (tests/topology_cases.py) without a GPU -- the oracle that judges every row, the descriptor round trip, the
packer on every row under ASan + UBSan, and the exact text of every refusal the table's REFUSED rows name.

The refusals all come from chiron_engine_plan or from pack_weights (both host-only), so a model the kernels do not cover never
reaches a kernel: chiron_engine_create runs both before its first GPU call."""
import os
import re
import subprocess

import numpy as np
import pytest

import chiron_amd as ca
from chiron_amd import _lib
from chiron_amd.engine import plan_sizes

import topology_cases as tc
from test_weight_pack_cpu import DTYPES, digest_exe          # noqa: F401  (the stand-alone ASan + UBSan packer program)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "chiron_amd", "csrc")
NAMES = [c.name for c in tc.CASES]


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_table_holds_every_row_of_its_plan():
    """the rows the table was written for are there, within the shape limits that keep a row at a second or two"""
    need = {"c128", "c64", "c320", "c192", "c36", "c12", "c4", "widen", "narrow", "last200-stack", "last200-multi", "last100-multi", "c576",
            "blocks1", "blocks2", "blocks5", "blocks8", "k1", "k2", "k4", "k5", "k16", "lift-k2", "lift-k16", "stride2-L126", "stride2-L127",
            "stride3-L126", "stride3-L127", "stride3-L128", "ibn-block2", "no-ibn-block1", "stem64-k1", "stem8-k64", "classes2", "classes3",
            "classes4", "batch-c192", "batch-c64", "batch-c48", "batch-c1024", "batch-c192-wrap"}
    need |= {"%s%d" % (k, n) for k in ("stack", "multi") for n in (1, 2, 4, 8)}
    assert need <= set(NAMES)
    for c in tc.CASES:
        T = c.spec.output_len(c.L)
        assert c.spec.hidden == 100 and c.dtype == "fp32", c.name
        if c.name != "batch-c192-wrap" and c.name != "c64-f4":
            assert c.B <= 5 and T <= 130, c.name
        assert c.max_beam == 0 or c.spec.classes == 5, c.name
    wrap = tc.BY_NAME["batch-c192-wrap"]
    assert wrap.B * wrap.spec.output_len(wrap.L) > 2048 * (256 // (192 // 4))     # bn_apply's grid x its rows per block
    assert {c.L % 2 for c in tc.CASES if c.name.startswith("stride2")} == {0, 1}
    assert {c.L % 3 for c in tc.CASES if c.name.startswith("stride3")} == {0, 1, 2}


def test_the_rules_are_the_sources():
    """the numbers tests/topology_cases.py predicts the forms with are the ones in the source"""
    k = _source("kernels.h")
    for name, value in (("PWL_TP", tc.PWL_TP), ("PWL_MAX_BP", tc.PWL_MAX_BP), ("PWL_MAX_S", tc.PWL_MAX_S), ("BN_BATCH_MAX_C", 1024),
                        ("GEMM_MAX_SEG", 16)):
        assert re.findall(r"constexpr int %s = (\d+);" % name, k) == [str(value)], name
    assert "return channels <= PWL_MAX_BP && (PWL_TP - 1) * stride + k <= PWL_MAX_S && channels % 4 == 0;" in k
    w = _source("weight_pack.h")
    assert "b.k == 3 && b.stride == 1 && (t % 2) == 0 && co % 64 == 0 && ci == co && !sw.no_winograd)" in w
    assert "if (!batch && !sw.no_pwl && pwl_covers(co, b.k, b.stride)) {" in w


@pytest.mark.parametrize("name", NAMES)
def test_oracle_and_descriptor_of_every_row(name):
    """the float32 oracle agrees with the float64 one to float32 accuracy (a yardstick that is neither zero nor broken), and the
    spec survives the trip through its checkpoint variables"""
    c = tc.BY_NAME[name]
    spec, w, x, sl, T = tc.inputs(name)
    assert (sl[:3] == [T, 1, 0][:len(sl)]).all() and sl.max() <= T
    f64, l64 = tc.reference(name)
    f32, l32 = tc.reference(name, "float32")
    assert f64.dtype == np.float64 and f32.dtype == np.float32
    assert f64.shape == (c.B, T, spec.blocks[-1]["out"]) and l64.shape == (c.B, T, spec.classes)
    assert np.isfinite(l64).all() and np.isfinite(l32).all()
    e = tc.yardstick(name)
    # float32 accuracy: far below the values, far above nothing.  Features after a stack of K <= 3 * 1024 sums, logits behind a head of gain 20
    fn = tc.window_errors(f64, f64)[1].max()
    ln = tc.window_errors(l64, l64, sl)[1].max()
    assert 0 < e["features"] < 1e-4 * fn, (e, fn)
    assert 0 < e["logits"] < 1e-3 * ln, (e, ln)
    strides = {b["name"]: b["stride"] for b in spec.blocks}
    if spec.stem:
        strides["conv_layer"] = spec.stem["stride"]
    back = ca.spec_from_variables({k: tuple(v) for k, v in spec.variables().items()}, strides=strides)
    assert back.to_dict() == spec.to_dict()
    assert list(back.blob_layout().items()) == list(spec.blob_layout().items())
    sz = plan_sizes(spec, c.B, c.L, max_beam=c.max_beam)
    assert sz["T"] == T and sz["ratio"] == c.L / T


def _pack(exe, tmp_path, spec, L, dtype, switches=""):
    with open(str(tmp_path / "desc"), "wb") as f:
        f.write(bytes(spec.to_c()))
    spec.pack(ca.synthetic_weights(spec, seed=tc.WEIGHT_SEED)).tofile(str(tmp_path / "blob"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    env.pop("LD_PRELOAD", None)
    r = subprocess.run([exe, str(tmp_path / "desc"), str(tmp_path / "blob"), str(L), str(DTYPES[dtype]), switches or "-"], capture_output=True,
                       text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return r.stdout.splitlines()


@pytest.mark.parametrize("name", NAMES)
def test_the_packer_on_every_row(digest_exe, tmp_path, name):   # noqa: F811
    """csrc/weight_pack.h packs the row under ASan + UBSan; its geometry is the spec's, its Winograd and table buffers follow the rule"""
    c = tc.BY_NAME[name]
    lines = _pack(digest_exe, tmp_path, c.spec, c.L, c.dtype)
    assert not [l for l in lines if l.startswith("refused")], lines[:3]
    T, C = c.spec.output_len(c.L), c.spec.blocks[-1]["out"]
    assert [l for l in lines if l.startswith("geometry T ")][0].startswith("geometry T %d C %d stem " % (T, C))
    geo = [l for l in lines if l.startswith("geometry block ")]
    assert len(geo) == len(c.spec.blocks)
    for g, b, (t_in, t_out) in zip(geo, c.spec.blocks, tc.block_lengths(c.spec, c.L)):
        assert (" c_in %d c %d k %d stride %d " % (b["in"], b["out"], b["k"], b["stride"])) in g, g
        assert (" t_in %d t_out %d " % (t_in, t_out)) in g, g
    wino = sorted(int(l.split(".")[0][5:]) for l in lines if re.match(r"block\d+\.wino_u ", l))
    assert wino == tc.wino_blocks(c.spec, c.L), (wino, name)
    assert bool([l for l in lines if l.startswith("block0.pwl_tab ")]) == tc.table_block(c.spec)
    lstm = [l for l in lines if l.startswith("geometry lstm ")]
    assert len(lstm) == c.spec.rnn_layers and lstm[0].startswith("geometry lstm in_w %d nproj 1 " % C)
    assert re.match(r"uploads (\d+) named \1$", lines[-1]), lines[-1]


@pytest.mark.parametrize("row", tc.REFUSED, ids=[r[0] for r in tc.REFUSED])
def test_refusals_with_their_texts(digest_exe, tmp_path, row):   # noqa: F811
    """what the descriptor accepts and no kernel covers is refused, with its reason, where the engine is planned or packed"""
    name, spec, dtype, max_beam, switches, where, text = row
    if where == "plan":
        with pytest.raises(_lib.ChironError) as e:
            plan_sizes(spec, 2, 30, dtype=dtype, max_beam=max_beam)
        assert e.value.status == _lib.ERR_INVALID
        assert str(e.value) == "libchiron_amd status 1: " + text
    else:
        plan_sizes(spec, 2, 400, dtype=dtype, max_beam=max_beam)       # the sizes are fine: the packer is what refuses
        lines = _pack(digest_exe, tmp_path, spec, 400, dtype, switches)
        assert lines == ["refused 1 " + text]


@pytest.mark.parametrize("row", tc.ADMITTED_BY_THE_PACKER, ids=[r[0] for r in tc.ADMITTED_BY_THE_PACKER])
def test_the_refusals_stop_where_the_kernels_start(digest_exe, tmp_path, row):   # noqa: F811
    name, spec, dtype, switches = row
    lines = _pack(digest_exe, tmp_path, spec, 500, dtype, switches)
    assert len(lines) > 10 and not [l for l in lines if l.startswith("refused")]


def test_batch_bn_kernels_leave_rows_of_other_blocks_alone():
    """bn_batch.hip: a block of 256 threads covers 256 / (C / 4) whole rows; the threads past them must not touch the next block's first
    row.  Both kernels say so in their row loops, and the launchers' grids are what tests/topology_cases.py sized the wrap row for."""
    s = _source("bn_batch.hip")
    assert s.count("for (long m = (long)blockIdx.x * rper + rsub; rsub < rper && m < M; m += (long)gridDim.x * rper) {") == 1     # bn_stats_kernel
    assert s.count("if (rsub >= rper) return;") == 1                                                                             # bn_apply_kernel
    assert "hipLaunchKernelGGL(bn_apply_kernel, dim3(2048), dim3(256)" in s and "hipLaunchKernelGGL(bn_stats_kernel, dim3(1024), dim3(256)" in s
