"""Labelled windows for validation: the reference's training-data reader, chiron/chiron_input.py read_raw_data_sets (:429-525),
read_label (:570-594) and read_raw (:630-678), for a folder of `.signal` + `.label` pairs (`.label`: "start end base" per line,
as `chiron export` writes it, chiron/utils/raw.py:100-125).

Restated for skip_start = 10 and k_mer = 1 only.  A window is the CONCATENATION of consecutive label spans of the signal while
they fit in seq_length samples, padded with the signal that follows the first span that did not fit (chiron_input.py:681-692
padding); a window is kept when it holds more than MIN_SIGNAL_PRO * seq_length samples and more than MIN_LABEL_LENGTH labels.
Like the reference, the spans after the last full window are dropped.

Deviations, both deliberate:
  * a label that ends at or past the signal's end makes the reference abort the whole run (chiron_input.py:658 assert, re-raised
    at :484-486); here the file is logged and skipped, like the repository's other readers;
  * files are taken in sorted order within each folder of the walk (os.walk's own order depends on the file system).
A label letter outside ACGT skips the file, as the reference's try/except around read_label does (:474-480).
"""
import logging
import os
from collections import namedtuple

import numpy as np

from . import signal_io

MIN_LABEL_LENGTH = 2      # chiron_input.py:28-29
MIN_SIGNAL_PRO = 0.3
SKIP_START = 10

RawLabels = namedtuple("RawLabels", "start length base")                 # chiron_input.py:27 raw_labels
LabelledSet = namedtuple("LabelledSet", "event event_length label label_length files")

logger = logging.getLogger("chiron_amd.labelled")
_BASES = {"A": 0, "C": 1, "G": 2, "T": 3, "a": 0, "c": 1, "g": 2, "t": 3}
SIG_NORMS = {"none": None, "median": signal_io.MEDIAN, "mean": signal_io.MEAN}


def read_label(file_path, skip_start=SKIP_START):
    """chiron_input.py:570-594 with window_n = 0: every line "start end base" except the first and last skip_start lines.
    Raises ValueError on a base outside ACGT (the reference's base2ind raises there too)."""
    with open(file_path, "r") as f:
        records = [line.split() for line in f]
    for r in records:
        if r[2] not in _BASES:
            raise ValueError("%s: base %r is not one of ACGT" % (file_path, r[2]))
    n = len(records)
    keep = [r for i, r in enumerate(records) if not (i < skip_start or i > n - skip_start - 1)]
    return RawLabels(start=[int(r[0]) for r in keep], length=[int(r[1]) - int(r[0]) for r in keep], base=[_BASES[r[2]] for r in keep])


def read_raw(raw_signal, raw_label, max_seq_length):
    """chiron_input.py:630-678 -> (event [n, max_seq_length] float32, event_length [n] int32, label list of lists, label_length [n] int32).
    Raises ValueError where the reference's assert fails (a span reaching the signal's end)."""
    sig = np.asarray(raw_signal, dtype=np.float32)
    signal_len = sig.shape[0]
    events, ev_len, labels, lab_len = [], [], [], []
    cur_event = []            # list of signal slices
    cur_len = 0
    cur_label = []
    for start, seg, base in zip(raw_label.start, raw_label.length, raw_label.base):
        if not start + seg < signal_len:
            raise ValueError("label span %d + %d reaches past the signal (%d samples)" % (start, seg, signal_len))
        if cur_len + seg < max_seq_length:
            cur_event.append(sig[start:start + seg])
            cur_label.append(base)
            cur_len += seg
        else:
            if cur_len > max_seq_length * MIN_SIGNAL_PRO and len(cur_label) > MIN_LABEL_LENGTH:
                row = np.zeros(max_seq_length, dtype=np.float32)
                body = np.concatenate(cur_event) if cur_event else np.zeros(0, dtype=np.float32)
                pad = sig[start + seg:start + seg + max_seq_length][:max_seq_length - cur_len]
                row[:cur_len] = body
                row[cur_len:cur_len + pad.shape[0]] = pad
                events.append(row)
                ev_len.append(cur_len)
                labels.append(list(cur_label))
                lab_len.append(len(cur_label))
            # a span of max_seq_length or more starts the next window on its own, as in the reference (it never passes the
            # length check and is replaced by the span after it)
            cur_event = [sig[start:start + seg]]
            cur_len = seg
            cur_label = [base]
    ev = np.stack(events) if events else np.zeros((0, max_seq_length), dtype=np.float32)
    return ev, np.asarray(ev_len, dtype=np.int32), labels, np.asarray(lab_len, dtype=np.int32)


def read_raw_data_sets(data_dir, seq_length=300, max_segments=None, sig_norm=None):
    """chiron_input.py:429-525 without the hdf5 cache: walk data_dir bottom-up, pair every X.signal with X.label, window each pair.
    max_segments: as the reference, checked after every tenth file read (file_count % 10 == 0); past it the windows are cut to
    max_segments and the rest of that folder is not read (the walk goes on with the next folder, as the reference's does).  sig_norm: None / signal_io.MEDIAN / signal_io.MEAN (or "none" / "median" / "mean")."""
    if isinstance(sig_norm, str):
        sig_norm = SIG_NORMS[sig_norm]
    events, ev_len, labels, lab_len, files = [], [], [], [], []
    file_count = 0
    for root, _dirs, names in os.walk(data_dir, topdown=False):
        for name in sorted(names):
            if not name.endswith(".signal"):
                continue
            stem = os.path.splitext(name)[0]
            signal = signal_io.read_signal(os.path.join(root, name), normalize=sig_norm)
            if len(signal) == 0:
                continue
            label_f = os.path.join(root, stem + ".label")
            try:
                lab = read_label(label_f)
            except (OSError, ValueError, IndexError) as e:
                logger.warning("Read the label %s fail. Skipped (%s)", label_f, e)
                continue
            try:
                ev, el, lb, ll = read_raw(signal, lab, seq_length)
            except ValueError as e:
                logger.warning("Extract label from %s fail, skipped: %s", label_f, e)
                continue
            events.append(ev)
            ev_len.append(el)
            labels.extend(lb)
            lab_len.append(ll)
            files.extend([os.path.join(root, name)] * len(lb))
            if file_count % 10 == 0 and max_segments is not None and len(labels) > max_segments:
                events, ev_len, lab_len = [np.concatenate(events)[:max_segments]], [np.concatenate(ev_len)[:max_segments]], \
                    [np.concatenate(lab_len)[:max_segments]]
                del labels[max_segments:], files[max_segments:]
                break
            file_count += 1
    ev = np.concatenate(events) if events else np.zeros((0, seq_length), dtype=np.float32)
    el = np.concatenate(ev_len) if ev_len else np.zeros(0, dtype=np.int32)
    ll = np.concatenate(lab_len) if lab_len else np.zeros(0, dtype=np.int32)
    return LabelledSet(ev, el, labels, ll, files)


def dense_labels(labels, label_length):
    """list of label lists -> int32 [n, max(label_length)] padded with 0 (the kernels read only label_len entries)."""
    n = len(labels)
    lmax = int(max(label_length)) if n else 0
    out = np.zeros((n, max(lmax, 1)), dtype=np.int32)
    for i, lab in enumerate(labels):
        out[i, :len(lab)] = lab
    return out
