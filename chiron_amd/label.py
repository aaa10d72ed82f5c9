"""Labels for training from the model's own logits: CTC forced alignment of reads to the sequences they are known to have.

`chiron call` leaves raw/<read>.signal and, when a fast5 carries a basecall, reference/<read>_ref.fastq.  This module runs each
read's windows through the engine, aligns the frame logits to the reference bases on the GPU (chiron_ctc_align,
csrc/ctc_align.hip: the best monotone path over the 2L+1 CTC states, banded, with traceback) and writes <read>.signal +
<read>.label pairs, the folders `validate`, `finetune` and `train` read (labelled.py).  The reference project gets these labels
from an outside resquiggler (chiron/utils/raw.py reads Tombo's tables); here nothing but this package is needed.

A banded alignment is the best path inside its band, not a certified optimum (include/chiron_amd.h); the report carries the band
each read stopped at and its mean log-probability per frame, which is what to filter on.  There is no CPU fallback."""
import json
import logging
import os

import numpy as np

from . import _lib

THREADS = _lib.LABEL_THREADS
LDS_SLOTS = _lib.LABEL_LDS_SLOTS          # widest band (in states) whose recursion rows the kernel keeps in LDS
MAX_FRAMES = _lib.LABEL_MAX_FRAMES
MAX_BASES = _lib.LABEL_MAX_BASES
STATUS_ALIGNED, STATUS_INFEASIBLE, STATUS_BAND_EXHAUSTED = 0, 1, 2
STATUS_NAMES = {0: "aligned", 1: "infeasible", 2: "band_exhausted"}
BAND0, MAX_BAND = 256, 8192               # the command's defaults

logger = logging.getLogger("chiron_amd.label")


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def workspace_size(frames, bases, band0, max_band):
    """chiron_ctc_align_workspace_size for reads of frames[r] frames and bases[r] bases (host-only)."""
    if len(frames) != len(bases):
        raise ValueError("%d frame counts against %d base counts" % (len(frames), len(bases)))
    fo, lo = _offsets(frames), _offsets(bases)
    return _lib.sized("chiron_ctc_align_workspace_size", len(frames), fo.ctypes.data, lo.ctypes.data, band0, max_band)


def plan_batches(frames, bases, band0, max_band, budget_bytes):
    """Lists of read indices, in input order, each list's workspace within budget_bytes; a read that alone exceeds the budget
    gets a batch of its own.  Uses only the host-only size function."""
    batches, cur = [], []
    for r in range(len(frames)):
        trial = cur + [r]
        if cur and workspace_size([frames[i] for i in trial], [bases[i] for i in trial], band0, max_band) > budget_bytes:
            batches.append(cur)
            trial = [r]
        cur = trial
    if cur:
        batches.append(cur)
    return batches


def align(scores_list, labels_list, band0=BAND0, max_band=MAX_BAND, device_id=0):
    """Align scores_list[r] (float32 [F_r, 5], class 4 = blank) to labels_list[r] (uint8 codes 0..3) on the GPU, all reads in
    one launch.  -> {"start": [int32 [L_r]] first frame of every base, "score": float64 [reads], "band": int32 [reads],
    "status": int32 [reads]} (0 aligned, 1 infeasible, 2 band exhausted; for 1 and 2 start is -1 and score -inf)."""
    if len(scores_list) != len(labels_list):
        raise ValueError("%d score arrays against %d label arrays" % (len(scores_list), len(labels_list)))
    reads = len(scores_list)
    xs = [np.ascontiguousarray(x, dtype=np.float32).reshape(-1, 5) for x in scores_list]
    ls = [np.ascontiguousarray(l, dtype=np.uint8).reshape(-1) for l in labels_list]
    score = np.zeros(reads, dtype=np.float64)
    band = np.zeros(reads, dtype=np.int32)
    status = np.zeros(reads, dtype=np.int32)
    if reads == 0:
        return {"start": [], "score": score, "band": band, "status": status}
    frame_off = _offsets([x.shape[0] for x in xs])
    label_off = _offsets([l.shape[0] for l in ls])
    scores = np.ascontiguousarray(np.concatenate(xs + [np.zeros((1, 5), np.float32)]))
    labels = np.ascontiguousarray(np.concatenate(ls + [np.zeros(1, np.uint8)]))
    start = np.full(int(label_off[-1]) + 1, -1, dtype=np.int32)
    lib, ws, stream = _lib.device_workspace(lambda: _lib.sized("chiron_ctc_align_workspace_size", reads, frame_off.ctypes.data,
                                                               label_off.ctypes.data, band0, max_band),
                                            device_id, "label.align", "alignment")
    _lib.check(lib.chiron_ctc_align(device_id, scores.ctypes.data, frame_off.ctypes.data, labels.ctypes.data, label_off.ctypes.data,
                                    reads, band0, max_band, 0, start.ctypes.data, score.ctypes.data, band.ctypes.data,
                                    status.ctypes.data, ws.data_ptr(), stream))
    del ws
    return {"start": [start[label_off[r]:label_off[r + 1]].copy() for r in range(reads)], "score": score, "band": band, "status": status}


def frames_to_samples(start_frames, seq_lens, segment_len, ratio, signal_len):
    """Frame indices of a read's concatenated valid frames -> sample positions.  The read was windowed without overlap (jump =
    segment_len) and window k contributed seq_lens[k] frames; local frame f of window k starts at sample k * segment_len +
    round(f * ratio), rounded half to even as seq_len_for_engine rounds, capped at signal_len."""
    start_frames = np.asarray(start_frames, dtype=np.int64)
    bounds = _offsets(seq_lens)
    if start_frames.size and (start_frames.min() < 0 or start_frames.max() >= bounds[-1]):
        raise ValueError("a frame index outside the read's %d frames" % bounds[-1])
    k = np.searchsorted(bounds, start_frames, side="right") - 1
    local = start_frames - bounds[k]
    pos = k * int(segment_len) + np.round(local.astype(np.float64) * ratio).astype(np.int64)
    return np.minimum(pos, int(signal_len))


def spans(start_samples, signal_len):
    """[(start, end)] per base: from its own start to the start of the next base, the last one to signal_len (the sample after
    the read's last frame).  Blank frames after a base belong to it; samples before the first base stay unlabelled.  Raises
    ValueError on a span of zero length (two bases starting in one sample: possible when a frame covers more than one sample)."""
    s = np.asarray(start_samples, dtype=np.int64)
    e = np.concatenate([s[1:], [int(signal_len)]]).astype(np.int64)
    if np.any(e <= s):
        j = int(np.flatnonzero(e <= s)[0])
        raise ValueError("base %d has an empty span (%d .. %d)" % (j, s[j], e[j]))
    return list(zip(s.tolist(), e.tolist()))


def write_label(path, span_list, bases):
    """One `start end base` line per base: what labelled.read_label reads."""
    if len(span_list) != len(bases):
        raise ValueError("%d spans against %d bases" % (len(span_list), len(bases)))
    with open(path, "w") as f:
        for (a, b), code in zip(span_list, bases):
            f.write("%d %d %s\n" % (a, b, "ACGT"[int(code)]))


def read_frames(engine, signal, batch_size):
    """The read's windows (no overlap) through the engine -> (logits float32 [frames, 5] of the valid frames, concatenated;
    seq_lens int32 per window)."""
    from .engine import seq_len_for_engine
    seg = engine.segment_len
    sig = np.asarray(signal, dtype=np.float32)
    n = (len(sig) + seg - 1) // seg
    x = np.zeros((n, seg), dtype=np.float32)
    lens = np.zeros(n, dtype=np.int64)
    for k in range(n):
        piece = sig[k * seg:(k + 1) * seg]
        x[k, :len(piece)] = piece
        lens[k] = len(piece)
    sl = seq_len_for_engine(lens, engine.ratio)
    parts = []
    for i in range(0, n, batch_size):
        res = engine.infer(x[i:i + batch_size], sl[i:i + batch_size], beam_width=0, want_prob=False, want_logits=True)
        for k in range(res.logits.shape[0]):
            parts.append(res.logits[k, :sl[i + k]])
    logits = np.concatenate(parts) if parts else np.zeros((0, 5), dtype=np.float32)
    return np.ascontiguousarray(logits, dtype=np.float32), sl


def mean_log_prob(logits, score):
    """The path's mean log-probability per frame: (score - sum over frames of log-sum-exp of the frame's logits) / F, float64."""
    x = np.asarray(logits, dtype=np.float64)
    if x.shape[0] == 0:
        return None
    m = x.max(axis=1)
    lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
    return float((score - lse.sum()) / x.shape[0])


def find_signals(input_path):
    """[(stem, path)] of <in>/raw/*.signal, or of *.signal directly under <in>."""
    raw = os.path.join(input_path, "raw")
    folder = raw if os.path.isdir(raw) else input_path
    return [(os.path.splitext(f)[0], os.path.join(folder, f)) for f in sorted(os.listdir(folder)) if f.endswith(".signal")]


def label(args):
    """The `label` command: signals + references -> <out>/<stem>.signal, <out>/<stem>.label and <out>/label_report.json."""
    from . import assess, fast5, model as model_mod, signal_io
    from .engine import Engine
    signals = find_signals(args.input)
    if not signals:
        raise ValueError("no .signal file under %s" % args.input)
    ref_path = args.reference
    if ref_path is None:
        ref_path = os.path.join(args.input, "reference")
        if not os.path.isdir(ref_path):
            raise ValueError("%s has no reference/ folder: give the references with -r" % args.input)
    refs = assess.load_references(ref_path)
    paired, unpaired = assess.pair_reads(dict(signals), refs)
    os.makedirs(args.output, exist_ok=True)
    spec, weights, _ = model_mod.load_model(args.model, allow_synthetic=args.synthetic_weights)
    per_read, todo = [], []
    with Engine(spec, weights, max_batch=args.batch_size, segment_len=args.segment_len, device_id=args.device, dtype=args.dtype) as eng:
        ratio = eng.ratio
        for stem, sig_path, ref in paired:
            codes = assess.encode(ref)                    # U is T in either mode
            if np.any(codes > 3):
                logger.warning("label: the reference of %s holds a base outside ACGT: skipped", stem)
                per_read.append({"name": stem, "bases": int(len(codes)), "status": "skipped", "reason": "reference holds a base outside ACGT"})
                continue
            signal = signal_io.read_signal(sig_path, normalize=signal_io.SIG_NORM)   # as `call` reads it
            logits, sl = read_frames(eng, signal, args.batch_size)
            todo.append({"name": stem, "signal": np.asarray(signal), "logits": logits, "seq_lens": sl, "codes": codes})
    frames = [t["logits"].shape[0] for t in todo]
    bases = [len(t["codes"]) for t in todo]
    totals = {name: 0 for name in STATUS_NAMES.values()}
    totals["skipped"] = sum(1 for r in per_read if r["status"] == "skipped")
    totals["written"] = 0
    for batch in plan_batches(frames, bases, args.band, args.max_band, args.workspace_mb << 20):
        got = align([todo[i]["logits"] for i in batch], [todo[i]["codes"] for i in batch], band0=args.band, max_band=args.max_band,
                    device_id=args.device)
        for k, i in enumerate(batch):
            t = todo[i]
            st = int(got["status"][k])
            rec = {"name": t["name"], "frames": frames[i], "bases": bases[i], "band": int(got["band"][k]), "status": STATUS_NAMES[st],
                   "score": float(got["score"][k]) if st == 0 else None,
                   "mean_log_prob": mean_log_prob(t["logits"], got["score"][k]) if st == 0 else None, "written": False}
            totals[STATUS_NAMES[st]] += 1
            if st == 0 and bases[i] > 0:
                n = len(t["signal"])
                try:
                    sp = spans(frames_to_samples(got["start"][k], t["seq_lens"], args.segment_len, ratio, n), n)
                except ValueError as e:
                    logger.warning("label: %s skipped: %s", t["name"], e)
                    rec["reason"] = str(e)
                else:
                    fast5.write_signal_text(os.path.join(args.output, t["name"] + ".signal"), t["signal"])
                    write_label(os.path.join(args.output, t["name"] + ".label"), sp, t["codes"])
                    rec["written"] = True
                    totals["written"] += 1
            per_read.append(rec)
    report = {"input": args.input, "reference": ref_path, "model": args.model, "segment_len": args.segment_len, "band": args.band,
              "max_band": args.max_band, "ratio": ratio, "totals": totals, "no_reference_count": len(unpaired),
              "no_reference": list(unpaired), "reads": sorted(per_read, key=lambda r: r["name"])}
    with open(os.path.join(args.output, "label_report.json"), "w") as f:
        json.dump(report, f, indent=1)
    return report
