"""CPU: the refusals the five alignment entry points share (csrc/align_common.h) -- chiron_align_pairs, chiron_align_infix,
chiron_align_trace, chiron_pileup and chiron_ctc_align.  One bad call per entry point and check; the status and the text of
chiron_last_error() are pinned byte for byte.  The expected strings were recorded from a build of the commit before the checks
were shared, so they say what the five separate copies said.  Every check precedes device use or stops at the missing device."""
import numpy as np
import pytest

from chiron_amd import _lib

CHECKS = ("negative_first_offset", "decreasing_offset", "over_long", "over_long_second", "code_out_of_range", "too_many_items", "unknown_flags",
          "null_workspace", "no_device")
TOO_MANY = (1 << 24) + 1

# per entry point: the arguments of a good one-item call, as a dict in the prototype's order, and what each check changes in it
READ = [0, 1, 2, 3]


def _pairs_args():
    return {"device_id": 0, "codes": np.array(READ + READ, np.uint8), "read_off": [0, 4], "ref_off": [4, 8], "pairs": 1, "flags": 0,
            "edit_out": np.zeros(1, np.int32), "match_out": np.zeros(1, np.int32), "band_out": np.zeros(1, np.int32),
            "workspace": np.zeros(64, np.uint8), "stream": None}


def _infix_args():
    return {"device_id": 0, "codes": np.array(READ + READ, np.uint8), "read_off": [0, 4], "win_off": [4, 8], "pairs": 1, "band0": 8,
            "flags": 0, "edit_out": np.zeros(1, np.int32), "match_out": np.zeros(1, np.int32), "start_out": np.zeros(1, np.int32),
            "end_out": np.zeros(1, np.int32), "band_out": np.zeros(1, np.int32), "workspace": np.zeros(64, np.uint8), "stream": None}


def _trace_args():
    return {"device_id": 0, "codes": np.array(READ + READ, np.uint8), "read_off": [0, 4], "ref_off": [4, 8], "pairs": 1,
            "edit_in": np.zeros(1, np.int32), "match_in": np.full(1, 4, np.int32), "ops_off": [0, 4], "flags": 0,
            "ops_out": np.zeros(4, np.uint8), "status_out": np.zeros(1, np.int32), "workspace": np.zeros(64, np.uint8), "stream": None}


def _pileup_args():
    return {"device_id": 0, "codes": np.array(READ, np.uint8), "read_off": [0, 4], "ops": np.zeros(4, np.uint8), "ops_off": [0, 4],
            "pos": [0], "alignments": 1, "g0": 0, "g1": 4, "ref_codes": np.array(READ, np.uint8), "min_depth": 1, "flags": 0,
            "counts_out": None, "depth_out": np.zeros(4, np.int32), "call_out": np.zeros(32, np.uint8), "clipped_out": np.zeros(1, np.int64),
            "workspace": np.zeros(64, np.uint8), "stream": None}


def _label_args():
    return {"device_id": 0, "scores": np.zeros(40, np.float32), "frame_off": [0, 8], "labels": np.array(READ, np.uint8),
            "label_off": [0, 4], "reads": 1, "band0": 8, "max_band": 0, "flags": 0, "start_out": np.zeros(4, np.int32),
            "score_out": np.zeros(1, np.float64), "band_out": np.zeros(1, np.int32), "status_out": np.zeros(1, np.int32),
            "workspace": np.zeros(64, np.uint8), "stream": None}


def _changes(count, first, second, long_len, long_second, codes, bad_code):
    """What each check changes: `first` / `second` name the two offset arrays, `codes` the code array."""
    return {"negative_first_offset": {first: [-1, 4]}, "decreasing_offset": {second: [6, 5]}, "over_long": {first: [0, long_len]},
            "over_long_second": {second: [0, long_second]},
            "code_out_of_range": {codes: np.array([0, 1, 2, bad_code], np.uint8)}, "too_many_items": {count: TOO_MANY},
            "unknown_flags": {"flags": 8}, "null_workspace": {"workspace": None}, "no_device": {"device_id": -1}}


ENTRIES = {
    "chiron_align_pairs": (_pairs_args, _changes("pairs", "read_off", "ref_off", _lib.ALIGN_MAX_LEN + 1, _lib.ALIGN_MAX_LEN + 1, "codes", 5)),
    "chiron_align_infix": (_infix_args, _changes("pairs", "read_off", "win_off", _lib.INFIX_MAX_READ + 1, _lib.INFIX_MAX_WINDOW + 1, "codes", 5)),
    "chiron_align_trace": (_trace_args, _changes("pairs", "read_off", "ref_off", _lib.ALIGN_MAX_LEN + 1, _lib.ALIGN_MAX_LEN + 1, "codes", 5)),
    "chiron_pileup": (_pileup_args, _changes("alignments", "read_off", "ops_off", _lib.PILEUP_MAX_COLUMNS + 1, _lib.PILEUP_MAX_COLUMNS + 1, "codes", 5)),
    "chiron_ctc_align": (_label_args, _changes("reads", "frame_off", "label_off", _lib.LABEL_MAX_FRAMES + 1, _lib.LABEL_MAX_BASES + 1, "labels", 4)),
}

EXPECTED = {
    ('chiron_align_infix', 'negative_first_offset'): (1, 'chiron_align_infix: read_off[0] = -1 is negative'),
    ('chiron_align_infix', 'decreasing_offset'): (1, 'chiron_align_infix: win_off[1] = 5 below its predecessor 6'),
    ('chiron_align_infix', 'over_long'): (4, 'chiron_align_infix: read 0 has 131073 bases, at most 131072'),
    ('chiron_align_infix', 'over_long_second'): (4, 'chiron_align_infix: window 0 has 1048576 bases, at most 1048575'),
    ('chiron_align_infix', 'code_out_of_range'): (1, 'chiron_align_infix: code 5 at 3 of read 0 outside 0..4'),
    ('chiron_align_infix', 'too_many_items'): (4, 'chiron_align_infix: 16777217 pairs in one call, at most 2^24'),
    ('chiron_align_infix', 'unknown_flags'): (1, 'chiron_align_infix: unknown flags 0x8'),
    ('chiron_align_infix', 'null_workspace'): (1, 'chiron_align_infix: null workspace'),
    ('chiron_align_infix', 'no_device'): (2, 'no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_align_pairs', 'negative_first_offset'): (1, 'chiron_align_pairs: read_off[0] = -1 is negative'),
    ('chiron_align_pairs', 'decreasing_offset'): (1, 'chiron_align_pairs: ref_off[1] = 5 below its predecessor 6'),
    ('chiron_align_pairs', 'over_long'): (4, 'chiron_align_pairs: read 0 has 131073 bases, at most 131072'),
    ('chiron_align_pairs', 'over_long_second'): (4, 'chiron_align_pairs: reference 0 has 131073 bases, at most 131072'),
    ('chiron_align_pairs', 'code_out_of_range'): (1, 'chiron_align_pairs: code 5 at 3 of read 0 outside 0..4'),
    ('chiron_align_pairs', 'too_many_items'): (4, 'chiron_align_pairs: 16777217 pairs in one call, at most 2^24'),
    ('chiron_align_pairs', 'unknown_flags'): (1, 'chiron_align_pairs: unknown flags 0x8'),
    ('chiron_align_pairs', 'null_workspace'): (1, 'chiron_align_pairs: null workspace'),
    ('chiron_align_pairs', 'no_device'): (2, 'no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_align_trace', 'negative_first_offset'): (1, 'chiron_align_trace: read_off[0] = -1 is negative'),
    ('chiron_align_trace', 'decreasing_offset'): (1, 'chiron_align_trace: ref_off[1] = 5 below its predecessor 6'),
    ('chiron_align_trace', 'over_long'): (4, 'chiron_align_trace: read 0 has 131073 bases, at most 131072'),
    ('chiron_align_trace', 'over_long_second'): (4, 'chiron_align_trace: reference 0 has 131073 bases, at most 131072'),
    ('chiron_align_trace', 'code_out_of_range'): (1, 'chiron_align_trace: code 5 at 3 of read 0 outside 0..4'),
    ('chiron_align_trace', 'too_many_items'): (4, 'chiron_align_trace: 16777217 pairs in one call, at most 2^24'),
    ('chiron_align_trace', 'unknown_flags'): (1, 'chiron_align_trace: unknown flags 0x8'),
    ('chiron_align_trace', 'null_workspace'): (1, 'chiron_align_trace: null workspace'),
    ('chiron_align_trace', 'no_device'): (2, 'no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_ctc_align', 'negative_first_offset'): (1, 'ctc_align: a negative first offset'),
    ('chiron_ctc_align', 'decreasing_offset'): (1, 'ctc_align: offsets of read 0 decrease'),
    ('chiron_ctc_align', 'over_long'): (4, 'ctc_align: read 0 has 16777217 frames, at most 16777216'),
    ('chiron_ctc_align', 'over_long_second'): (4, 'ctc_align: read 0 has 4194305 bases, at most 4194304'),
    ('chiron_ctc_align', 'code_out_of_range'): (1, 'chiron_ctc_align: code 4 at base 3 outside 0..3'),
    ('chiron_ctc_align', 'too_many_items'): (4, 'ctc_align: 16777217 reads in one call, at most 2^24'),
    ('chiron_ctc_align', 'unknown_flags'): (1, 'chiron_ctc_align: unknown flags 0x8'),
    ('chiron_ctc_align', 'null_workspace'): (1, 'chiron_ctc_align: null workspace'),
    ('chiron_ctc_align', 'no_device'): (2, 'no HIP device -1: libchiron_amd has no CPU fallback'),
    ('chiron_pileup', 'negative_first_offset'): (1, 'chiron_pileup: read_off[0] = -1 is negative'),
    ('chiron_pileup', 'decreasing_offset'): (1, 'chiron_pileup: ops_off[1] = 5 below its predecessor 6'),
    ('chiron_pileup', 'over_long'): (4, 'chiron_pileup: alignment 0 has 16777217 read bases, at most 16777216'),
    ('chiron_pileup', 'over_long_second'): (4, 'chiron_pileup: alignment 0 has 16777217 columns, at most 16777216'),
    ('chiron_pileup', 'code_out_of_range'): (1, 'chiron_pileup: code 5 at 3 of read 0 outside 0..4'),
    ('chiron_pileup', 'too_many_items'): (4, 'chiron_pileup: 16777217 alignments in one call, at most 2^24'),
    ('chiron_pileup', 'unknown_flags'): (1, 'chiron_pileup: unknown flags 0x8'),
    ('chiron_pileup', 'null_workspace'): (1, 'chiron_pileup: null workspace'),
    ('chiron_pileup', 'no_device'): (2, 'no HIP device -1: libchiron_amd has no CPU fallback'),
}


def refuse(lib, entry, check):
    """(status, message) of `entry`'s good call with `check`'s change applied."""
    make, changes = ENTRIES[entry]
    args = make()
    args.update(changes[check])
    keep = [np.asarray(v, dtype=np.int64) if isinstance(v, list) else v for v in args.values()]
    raw = [v.ctypes.data if isinstance(v, np.ndarray) else v for v in keep]
    status = getattr(lib, entry)(*raw)
    return status, lib.chiron_last_error().decode()


@pytest.mark.parametrize("check", CHECKS)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_refusal_status_and_text(built, entry, check):
    assert refuse(_lib.load(), entry, check) == EXPECTED[entry, check]
