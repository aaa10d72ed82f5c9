"""CPU: the library's one reading of the weight blob and of the convolution geometry (csrc/model_layout.h).

(a) For every topology of model.py the section edges the library reports -- chiron_cnn_params_range, chiron_rnn_params_range,
    chiron_weights_size -- tile ModelSpec.blob_layout() exactly.  (DNA_default, RNA_default and the two stem models in population
    mode are also in test_train_cpu.py / test_cnn_train_cpu.py, which check the layouts inside the sections on the Python side.)
(b) Every refusal of the entry points that read the descriptor which can be provoked without a GPU: status and the text of
    chiron_last_error(), pinned byte for byte.  The expected strings were recorded from a build of the commit before the layout was
    shared, so they say what the separate walkers said.  Every check precedes device use or stops at the missing device.
    (The CNN seam's own "multiples of 4" refusal cannot be reached: the descriptor check refuses such channels first.)"""
import ctypes as C

import numpy as np
import pytest

import chiron_amd as ca
from chiron_amd import _lib, train


# ---------------------------------------------------------------------------------------------
# (a) the sections tile the blob
# ---------------------------------------------------------------------------------------------
def _multi_dna(bn_mode):
    spec = ca.dna_default_spec(bn_mode)
    return ca.ModelSpec(spec.blocks, "multi", 4, 100, 5, bn_mode)


SPECS = {"dna": ca.dna_default_spec, "rna": ca.rna_default_spec, "rna_model2": lambda bn: ca.rna_head_spec("rna_model2", bn),
         "rna_model3": lambda bn: ca.rna_head_spec("rna_model3", bn), "dna_multi4": _multi_dna}


@pytest.mark.parametrize("bn_mode", ["population", "batch"])
@pytest.mark.parametrize("kind", sorted(SPECS))
def test_the_sections_the_library_reports_tile_blob_layout(built, kind, bn_mode):
    spec = SPECS[kind](bn_mode)
    layout = spec.blob_layout()
    names = list(layout)
    sizes = [int(np.prod(s)) for s in layout.values()]
    n_cnn = sum(sizes[:names.index(spec.lstm_scope(0, "fw") + "kernel")])
    assert train.cnn_params_range(spec) == (0, n_cnn)
    assert train.params_range(spec) == (n_cnn, sum(sizes) - n_cnn)
    assert _lib.sized("chiron_weights_size", C.byref(spec.to_c())) == sum(sizes) == len(spec.pack(ca.synthetic_weights(spec, seed=1)))


# ---------------------------------------------------------------------------------------------
# (b) refusals
# ---------------------------------------------------------------------------------------------
def _buf():
    return np.zeros(16, np.float32)


# per entry point: the arguments of a good call on DNA_default, in the prototype's order ("desc" is filled in by refuse()).  The four
# that launch are given host memory and device -1: what passes their host checks stops at the missing device, with or without a GPU.
def _out2():
    return {"a": C.c_size_t(), "b": C.c_size_t()}


ENTRIES = {
    "chiron_weights_size": lambda: {"desc": None, "n_floats": C.c_size_t()},
    "chiron_rnn_params_range": lambda: dict(desc=None, **_out2()),
    "chiron_cnn_params_range": lambda: dict(desc=None, **_out2()),
    "chiron_rnn_train_sizes": lambda: dict(desc=None, batch=16, T=12, **_out2()),
    "chiron_cnn_train_sizes": lambda: dict(desc=None, batch=3, segment_len=40, **_out2()),
    "chiron_cnn_train_tape_relu": lambda: {"desc": None, "batch": 3, "segment_len": 40, "index": 0, "offset": C.c_size_t(),
                                           "frames": C.c_int32(), "channels": C.c_int32()},
    "chiron_engine_plan": lambda: {"desc": None, "opts": _lib.EngineOpts(0, 16, 400, 1, 0, 0), "out": _lib.EngineSizes()},
    "chiron_rnn_train_forward": lambda: {"device_id": -1, "desc": None, "params": _buf(), "features": _buf(), "seq_len": _buf(), "batch": 16,
                                         "T": 12, "logits_out": _buf(), "tape": _buf(), "workspace": _buf(), "stream": None},
    "chiron_rnn_train_backward": lambda: {"device_id": -1, "desc": None, "params": _buf(), "features": _buf(), "seq_len": _buf(),
                                          "dlogits": _buf(), "batch": 16, "T": 12, "tape": _buf(), "workspace": _buf(),
                                          "dparams_out": _buf(), "dfeatures_out": None, "stream": None},
    "chiron_cnn_train_forward": lambda: {"device_id": -1, "desc": None, "params": _buf(), "signal": _buf(), "batch": 3, "segment_len": 40,
                                         "features_out": _buf(), "moments_out": _buf(), "tape": _buf(), "workspace": _buf(), "stream": None},
    "chiron_cnn_train_backward": lambda: {"device_id": -1, "desc": None, "params": _buf(), "signal": _buf(), "dfeatures": _buf(), "batch": 3,
                                          "segment_len": 40, "tape": _buf(), "workspace": _buf(), "dparams_out": _buf(), "stream": None},
}
TRAINING = [e for e in ENTRIES if e.endswith("ward")]
RNN_SHAPED = ["chiron_rnn_train_sizes", "chiron_rnn_train_forward", "chiron_rnn_train_backward"]
CNN_SHAPED = ["chiron_cnn_train_sizes", "chiron_cnn_train_tape_relu", "chiron_cnn_train_forward", "chiron_cnn_train_backward"]


def _block(i, **kw):
    def change(d):
        for k, v in kw.items():
            setattr(d.blocks[i], k, v)
    return change


def _channels(c, first=1):
    def change(d):   # c channels from block `first`'s input on
        for i in range(3):
            if i >= first:
                d.blocks[i].in_channels = c
            if i >= first - 1:
                d.blocks[i].out_channels = c
    return change


def _stem(d):   # a 65-wide stem in front of consistent blocks
    d.stem_k, d.stem_stride, d.stem_channels, d.blocks[0].in_channels = 65, 1, 8, 8


# what each descriptor check changes in DNA_default's descriptor: one per clause of the descriptor check, then what only the
# training kernels refuse
DESC_CHECKS = {
    "n_blocks": lambda d: setattr(d, "n_blocks", 0),
    "in_channels": _block(1, in_channels=128),
    "out_channels": _block(2, out_channels=254),
    "conv2b_width": _block(0, k=17),
    "stride": _block(0, stride=0),
    "stem": _stem,
    "rnn_kind": lambda d: setattr(d, "rnn_kind", 7),
    "rnn_layers": lambda d: setattr(d, "rnn_layers", 9),
    "hidden": lambda d: setattr(d, "hidden", 98),
    "classes": lambda d: setattr(d, "classes", 6),
    "bn_mode": lambda d: setattr(d, "bn_mode", 5),
    "hidden_96": lambda d: setattr(d, "hidden", 96),
    "classes_4": lambda d: setattr(d, "classes", 4),
    "channels_2052": _channels(2052, 2),
}

# what every other check changes in the good call's arguments ("change_desc": in its descriptor as well)
ARG_CHECKS = {e: {"null_desc": {"desc": "null"}} for e in ENTRIES}
ARG_CHECKS["chiron_weights_size"]["null_output"] = {"n_floats": None}
for e in ("chiron_rnn_params_range", "chiron_cnn_params_range", "chiron_rnn_train_sizes", "chiron_cnn_train_sizes"):
    ARG_CHECKS[e]["null_output"] = {"b": None}
ARG_CHECKS["chiron_cnn_train_tape_relu"].update({"null_output": {"frames": None}, "index_past_the_last": {"index": 10}, "index_negative": {"index": -1}})
for e in RNN_SHAPED:
    ARG_CHECKS[e].update({"batch_0": {"batch": 0}, "T_0": {"T": 0}, "batch_over": {"batch": (1 << 20) + 1}, "T_over": {"T": _lib.CTC_MAX_T + 1},
                          "rows_over": {"batch": 1 << 12, "T": (1 << 12) + 1}})
for e in CNN_SHAPED:
    ARG_CHECKS[e].update({"batch_0": {"batch": 0}, "segment_len_0": {"segment_len": 0}, "batch_over": {"batch": (1 << 20) + 1},
                          "segment_len_over": {"batch": 1, "segment_len": (1 << 24) + 1}, "rows_over": {"batch": 1 << 12, "segment_len": (1 << 12) + 1},
                          "frames_over": {"batch": 1, "segment_len": _lib.CTC_MAX_T + 1}})
ARG_CHECKS["chiron_engine_plan"].update({
    "null_opts": {"opts": None}, "null_output": {"out": None}, "max_batch_0": {"opts": _lib.EngineOpts(0, 0, 400, 1, 0, 0)},
    "segment_len_0": {"opts": _lib.EngineOpts(0, 16, 0, 1, 0, 0)}, "dtype": {"opts": _lib.EngineOpts(0, 16, 400, 1, 9, 0)},
    "max_beam": {"opts": _lib.EngineOpts(0, 16, 400, 1, 0, -1)}, "rows_over": {"opts": _lib.EngineOpts(0, 1 << 30, 400, 1, 0, 0)},
    "activation_over": {"opts": _lib.EngineOpts(0, 1 << 14, 400, 1, 0, 0)}, "lasth_over": {"opts": _lib.EngineOpts(0, 1 << 14, 400, 1, 0, 0), "change_desc": _channels(64)}})
for e in TRAINING:
    ARG_CHECKS[e].update({"null_operand": {"params": None}, "null_workspace": {"workspace": None}, "no_device": {}})

CASES = [(e, c) for e in ENTRIES for c in list(DESC_CHECKS) + list(ARG_CHECKS[e])]


def refuse(lib, entry, check):
    """(status, message) of `entry`'s good call with `check`'s change applied; the message of an accepted call is None."""
    args = ENTRIES[entry]()
    desc = ca.dna_default_spec().to_c()
    if check in DESC_CHECKS:
        DESC_CHECKS[check](desc)
    else:
        args.update(ARG_CHECKS[entry][check])
        args.pop("change_desc", lambda d: None)(desc)
    args["desc"] = None if args["desc"] == "null" else desc
    raw = [v.ctypes.data if isinstance(v, np.ndarray) else C.byref(v) if isinstance(v, (C.Structure, C._SimpleCData)) else v
           for v in args.values()]
    status = getattr(lib, entry)(*raw)
    return status, lib.chiron_last_error().decode() if status else None


EXPECTED = {
    ('chiron_weights_size', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_weights_size', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_weights_size', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_weights_size', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_weights_size', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_weights_size', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_weights_size', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_weights_size', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_weights_size', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_weights_size', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_weights_size', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_weights_size', 'hidden_96'): (0, None),
    ('chiron_weights_size', 'classes_4'): (0, None),
    ('chiron_weights_size', 'channels_2052'): (0, None),
    ('chiron_weights_size', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_weights_size', 'null_output'): (1, 'null n_floats'),
    ('chiron_rnn_params_range', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_rnn_params_range', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_rnn_params_range', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_rnn_params_range', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_rnn_params_range', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_rnn_params_range', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_rnn_params_range', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_rnn_params_range', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_rnn_params_range', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_rnn_params_range', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_rnn_params_range', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_rnn_params_range', 'hidden_96'): (1, 'the training kernels are built for hidden 100, not 96'),
    ('chiron_rnn_params_range', 'classes_4'): (1, 'the training kernels are built for 5 classes, not 4'),
    ('chiron_rnn_params_range', 'channels_2052'): (0, None),
    ('chiron_rnn_params_range', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_rnn_params_range', 'null_output'): (1, 'chiron_rnn_params_range: null output'),
    ('chiron_cnn_params_range', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_cnn_params_range', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_cnn_params_range', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_cnn_params_range', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_cnn_params_range', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_cnn_params_range', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_cnn_params_range', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_cnn_params_range', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_cnn_params_range', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_cnn_params_range', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_cnn_params_range', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_cnn_params_range', 'hidden_96'): (0, None),
    ('chiron_cnn_params_range', 'classes_4'): (0, None),
    ('chiron_cnn_params_range', 'channels_2052'): (1, 'the CNN training kernels take at most 2048 channels, not 2052'),
    ('chiron_cnn_params_range', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_cnn_params_range', 'null_output'): (1, 'chiron_cnn_params_range: null output'),
    ('chiron_rnn_train_sizes', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_rnn_train_sizes', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_rnn_train_sizes', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_rnn_train_sizes', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_rnn_train_sizes', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_rnn_train_sizes', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_rnn_train_sizes', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_rnn_train_sizes', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_rnn_train_sizes', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_rnn_train_sizes', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_rnn_train_sizes', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_rnn_train_sizes', 'hidden_96'): (1, 'the training kernels are built for hidden 100, not 96'),
    ('chiron_rnn_train_sizes', 'classes_4'): (1, 'the training kernels are built for 5 classes, not 4'),
    ('chiron_rnn_train_sizes', 'channels_2052'): (0, None),
    ('chiron_rnn_train_sizes', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_rnn_train_sizes', 'null_output'): (1, 'chiron_rnn_train_sizes: null output'),
    ('chiron_rnn_train_sizes', 'batch_0'): (1, 'batch 0, T 12: both must be positive'),
    ('chiron_rnn_train_sizes', 'T_0'): (1, 'batch 16, T 0: both must be positive'),
    ('chiron_rnn_train_sizes', 'batch_over'): (4, "batch 1048577 / T 12 beyond the training kernels' range (2^20 rows, 8192 frames)"),
    ('chiron_rnn_train_sizes', 'T_over'): (4, "batch 16 / T 8193 beyond the training kernels' range (2^20 rows, 8192 frames)"),
    ('chiron_rnn_train_sizes', 'rows_over'): (4, 'T * padded batch = 16781312 rows: the training kernels index at most 2^24'),
    ('chiron_cnn_train_sizes', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_cnn_train_sizes', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_cnn_train_sizes', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_cnn_train_sizes', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_cnn_train_sizes', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_cnn_train_sizes', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_cnn_train_sizes', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_cnn_train_sizes', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_cnn_train_sizes', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_cnn_train_sizes', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_cnn_train_sizes', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_cnn_train_sizes', 'hidden_96'): (0, None),
    ('chiron_cnn_train_sizes', 'classes_4'): (0, None),
    ('chiron_cnn_train_sizes', 'channels_2052'): (1, 'the CNN training kernels take at most 2048 channels, not 2052'),
    ('chiron_cnn_train_sizes', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_cnn_train_sizes', 'null_output'): (1, 'chiron_cnn_train_sizes: null output'),
    ('chiron_cnn_train_sizes', 'batch_0'): (1, 'batch 0, segment_len 40: both must be positive'),
    ('chiron_cnn_train_sizes', 'segment_len_0'): (1, 'batch 3, segment_len 0: both must be positive'),
    ('chiron_cnn_train_sizes', 'batch_over'): (4, "batch 1048577 x segment_len 40 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_sizes', 'segment_len_over'): (4, "batch 1 x segment_len 16777217 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_sizes', 'rows_over'): (4, "batch 4096 x segment_len 4097 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_sizes', 'frames_over'): (4, '8193 frames: the training kernels take at most 8192'),
    ('chiron_cnn_train_tape_relu', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_cnn_train_tape_relu', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_cnn_train_tape_relu', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_cnn_train_tape_relu', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_cnn_train_tape_relu', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_cnn_train_tape_relu', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_cnn_train_tape_relu', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_cnn_train_tape_relu', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_cnn_train_tape_relu', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_cnn_train_tape_relu', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_cnn_train_tape_relu', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_cnn_train_tape_relu', 'hidden_96'): (0, None),
    ('chiron_cnn_train_tape_relu', 'classes_4'): (0, None),
    ('chiron_cnn_train_tape_relu', 'channels_2052'): (1, 'the CNN training kernels take at most 2048 channels, not 2052'),
    ('chiron_cnn_train_tape_relu', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_cnn_train_tape_relu', 'null_output'): (1, 'chiron_cnn_train_tape_relu: null output'),
    ('chiron_cnn_train_tape_relu', 'index_past_the_last'): (1, 'chiron_cnn_train_tape_relu: index 10 outside the 9 ReLU outputs'),
    ('chiron_cnn_train_tape_relu', 'index_negative'): (1, 'chiron_cnn_train_tape_relu: index -1 outside the 9 ReLU outputs'),
    ('chiron_cnn_train_tape_relu', 'batch_0'): (1, 'batch 0, segment_len 40: both must be positive'),
    ('chiron_cnn_train_tape_relu', 'segment_len_0'): (1, 'batch 3, segment_len 0: both must be positive'),
    ('chiron_cnn_train_tape_relu', 'batch_over'): (4, "batch 1048577 x segment_len 40 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_tape_relu', 'segment_len_over'): (4, "batch 1 x segment_len 16777217 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_tape_relu', 'rows_over'): (4, "batch 4096 x segment_len 4097 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_tape_relu', 'frames_over'): (4, '8193 frames: the training kernels take at most 8192'),
    ('chiron_engine_plan', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_engine_plan', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_engine_plan', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_engine_plan', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_engine_plan', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_engine_plan', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_engine_plan', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_engine_plan', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_engine_plan', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_engine_plan', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_engine_plan', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_engine_plan', 'hidden_96'): (0, None),
    ('chiron_engine_plan', 'classes_4'): (0, None),
    ('chiron_engine_plan', 'channels_2052'): (0, None),
    ('chiron_engine_plan', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_engine_plan', 'null_opts'): (1, 'null opts'),
    ('chiron_engine_plan', 'null_output'): (1, 'null out'),
    ('chiron_engine_plan', 'max_batch_0'): (1, 'max_batch/segment_len must be positive'),
    ('chiron_engine_plan', 'segment_len_0'): (1, 'max_batch/segment_len must be positive'),
    ('chiron_engine_plan', 'dtype'): (1, 'dtype 9 unknown (0 = f32, 1 = f16, 2 = f32 as hi/lo half pairs, 3 = f16 activations against hi/lo weights)'),
    ('chiron_engine_plan', 'max_beam'): (1, 'max_beam -1'),
    ('chiron_engine_plan', 'rows_over'): (4, "max_batch 1073741824 x 400 frames does not fit the kernels' int row index"),
    ('chiron_engine_plan', 'activation_over'): (4, 'max_batch 16384: an activation tensor [16384 x 400 x 256] needs 6710886400 bytes, the kernels address at most 4294836224 per tensor (about 10485 windows at this segment length and dtype): use a smaller max_batch'),
    ('chiron_engine_plan', 'lasth_over'): (4, 'max_batch 16384: the recurrent output [400 x 16384 x 200] needs 5242880000 bytes, the kernels address at most 4294836224 per tensor'),
    ('chiron_rnn_train_forward', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_rnn_train_forward', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_rnn_train_forward', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_rnn_train_forward', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_rnn_train_forward', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_rnn_train_forward', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_rnn_train_forward', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_rnn_train_forward', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_rnn_train_forward', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_rnn_train_forward', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_rnn_train_forward', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_rnn_train_forward', 'hidden_96'): (1, 'the training kernels are built for hidden 100, not 96'),
    ('chiron_rnn_train_forward', 'classes_4'): (1, 'the training kernels are built for 5 classes, not 4'),
    ('chiron_rnn_train_forward', 'channels_2052'): (2, 'chiron_rnn_train_forward: no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_rnn_train_forward', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_rnn_train_forward', 'batch_0'): (1, 'batch 0, T 12: both must be positive'),
    ('chiron_rnn_train_forward', 'T_0'): (1, 'batch 16, T 0: both must be positive'),
    ('chiron_rnn_train_forward', 'batch_over'): (4, "batch 1048577 / T 12 beyond the training kernels' range (2^20 rows, 8192 frames)"),
    ('chiron_rnn_train_forward', 'T_over'): (4, "batch 16 / T 8193 beyond the training kernels' range (2^20 rows, 8192 frames)"),
    ('chiron_rnn_train_forward', 'rows_over'): (4, 'T * padded batch = 16781312 rows: the training kernels index at most 2^24'),
    ('chiron_rnn_train_forward', 'null_operand'): (1, 'chiron_rnn_train_forward: null operand'),
    ('chiron_rnn_train_forward', 'null_workspace'): (1, 'chiron_rnn_train_forward: null operand'),
    ('chiron_rnn_train_forward', 'no_device'): (2, 'chiron_rnn_train_forward: no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_rnn_train_backward', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_rnn_train_backward', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_rnn_train_backward', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_rnn_train_backward', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_rnn_train_backward', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_rnn_train_backward', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_rnn_train_backward', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_rnn_train_backward', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_rnn_train_backward', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_rnn_train_backward', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_rnn_train_backward', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_rnn_train_backward', 'hidden_96'): (1, 'the training kernels are built for hidden 100, not 96'),
    ('chiron_rnn_train_backward', 'classes_4'): (1, 'the training kernels are built for 5 classes, not 4'),
    ('chiron_rnn_train_backward', 'channels_2052'): (2, 'chiron_rnn_train_backward: no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_rnn_train_backward', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_rnn_train_backward', 'batch_0'): (1, 'batch 0, T 12: both must be positive'),
    ('chiron_rnn_train_backward', 'T_0'): (1, 'batch 16, T 0: both must be positive'),
    ('chiron_rnn_train_backward', 'batch_over'): (4, "batch 1048577 / T 12 beyond the training kernels' range (2^20 rows, 8192 frames)"),
    ('chiron_rnn_train_backward', 'T_over'): (4, "batch 16 / T 8193 beyond the training kernels' range (2^20 rows, 8192 frames)"),
    ('chiron_rnn_train_backward', 'rows_over'): (4, 'T * padded batch = 16781312 rows: the training kernels index at most 2^24'),
    ('chiron_rnn_train_backward', 'null_operand'): (1, 'chiron_rnn_train_backward: null operand'),
    ('chiron_rnn_train_backward', 'null_workspace'): (1, 'chiron_rnn_train_backward: null operand'),
    ('chiron_rnn_train_backward', 'no_device'): (2, 'chiron_rnn_train_backward: no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_cnn_train_forward', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_cnn_train_forward', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_cnn_train_forward', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_cnn_train_forward', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_cnn_train_forward', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_cnn_train_forward', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_cnn_train_forward', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_cnn_train_forward', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_cnn_train_forward', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_cnn_train_forward', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_cnn_train_forward', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_cnn_train_forward', 'hidden_96'): (2, 'chiron_cnn_train_forward: no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_cnn_train_forward', 'classes_4'): (2, 'chiron_cnn_train_forward: no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_cnn_train_forward', 'channels_2052'): (1, 'the CNN training kernels take at most 2048 channels, not 2052'),
    ('chiron_cnn_train_forward', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_cnn_train_forward', 'batch_0'): (1, 'batch 0, segment_len 40: both must be positive'),
    ('chiron_cnn_train_forward', 'segment_len_0'): (1, 'batch 3, segment_len 0: both must be positive'),
    ('chiron_cnn_train_forward', 'batch_over'): (4, "batch 1048577 x segment_len 40 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_forward', 'segment_len_over'): (4, "batch 1 x segment_len 16777217 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_forward', 'rows_over'): (4, "batch 4096 x segment_len 4097 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_forward', 'frames_over'): (4, '8193 frames: the training kernels take at most 8192'),
    ('chiron_cnn_train_forward', 'null_operand'): (1, 'chiron_cnn_train_forward: null operand'),
    ('chiron_cnn_train_forward', 'null_workspace'): (1, 'chiron_cnn_train_forward: null operand'),
    ('chiron_cnn_train_forward', 'no_device'): (2, 'chiron_cnn_train_forward: no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_cnn_train_backward', 'n_blocks'): (1, 'n_blocks 0 out of range'),
    ('chiron_cnn_train_backward', 'in_channels'): (1, 'block 1: in_channels 128, expected 256'),
    ('chiron_cnn_train_backward', 'out_channels'): (1, 'block 2: out_channels must be a multiple of 4'),
    ('chiron_cnn_train_backward', 'conv2b_width'): (1, 'block 0: conv2b width 17 unsupported (1..16)'),
    ('chiron_cnn_train_backward', 'stride'): (1, 'block 0: stride 0'),
    ('chiron_cnn_train_backward', 'stem'): (1, 'stem: k 65 stride 1 channels 8'),
    ('chiron_cnn_train_backward', 'rnn_kind'): (1, 'rnn_kind 7'),
    ('chiron_cnn_train_backward', 'rnn_layers'): (1, 'rnn_layers 9 unsupported (1..8)'),
    ('chiron_cnn_train_backward', 'hidden'): (1, 'hidden 98 unsupported (multiple of 4, <= 100)'),
    ('chiron_cnn_train_backward', 'classes'): (1, 'classes 6 unsupported (2..5)'),
    ('chiron_cnn_train_backward', 'bn_mode'): (1, 'bn_mode 5'),
    ('chiron_cnn_train_backward', 'hidden_96'): (2, 'chiron_cnn_train_backward: no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_cnn_train_backward', 'classes_4'): (2, 'chiron_cnn_train_backward: no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_cnn_train_backward', 'channels_2052'): (1, 'the CNN training kernels take at most 2048 channels, not 2052'),
    ('chiron_cnn_train_backward', 'null_desc'): (1, 'null model descriptor'),
    ('chiron_cnn_train_backward', 'batch_0'): (1, 'batch 0, segment_len 40: both must be positive'),
    ('chiron_cnn_train_backward', 'segment_len_0'): (1, 'batch 3, segment_len 0: both must be positive'),
    ('chiron_cnn_train_backward', 'batch_over'): (4, "batch 1048577 x segment_len 40 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_backward', 'segment_len_over'): (4, "batch 1 x segment_len 16777217 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_backward', 'rows_over'): (4, "batch 4096 x segment_len 4097 beyond the training kernels' range (batch 2^20, 2^24 rows)"),
    ('chiron_cnn_train_backward', 'frames_over'): (4, '8193 frames: the training kernels take at most 8192'),
    ('chiron_cnn_train_backward', 'null_operand'): (1, 'chiron_cnn_train_backward: null operand'),
    ('chiron_cnn_train_backward', 'null_workspace'): (1, 'chiron_cnn_train_backward: null operand'),
    ('chiron_cnn_train_backward', 'no_device'): (2, 'chiron_cnn_train_backward: no HIP device -1: libchiron_amd has no CPU fallback'),
}


def test_the_table_covers_every_case():
    assert sorted(EXPECTED) == sorted(CASES)


@pytest.mark.parametrize("entry,check", CASES)
def test_refusal_status_and_text(built, entry, check):
    assert refuse(_lib.load(), entry, check) == EXPECTED[entry, check]
