#!/usr/bin/env python3
"""Generate tests/golden/labelled_windows.json: the reference's labelled reader (chiron_input.read_label with skip_start=10,
k_mer=1, and read_raw) run on small synthetic .signal / .label pairs.  Runs only where the reference tree exists (see
make_golden.py); only the inputs and the reference's outputs are written, as data.

    python tests/golden/make_labelled_golden.py

The pairs cover gaps between label spans, windows rejected by the 0.3 signal share and by the label count (more than 2
needed), padding from the signal that follows, padding that the signal's end cuts short so that zeros fill the rest of the
window (zero_fill), and a span longer than the window.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


def make_cases():
    rng = np.random.default_rng(20261016)
    cases = []

    def case(name, n_sig, spans, seq_length):
        sig = rng.integers(300, 700, n_sig).tolist()
        lines = ["%d %d %s" % (a, b, "ACGT"[int(rng.integers(0, 4))]) for a, b in spans]
        cases.append({"name": name, "signal": sig, "label_lines": lines, "seq_length": seq_length})

    # contiguous spans of 3..12 samples
    pos, spans = 5, []
    while pos < 1900:
        n = int(rng.integers(3, 13))
        spans.append((pos, pos + n))
        pos += n
    case("contiguous", 2000, spans, 100)
    # gaps between spans
    pos, spans = 0, []
    while pos < 1400:
        n = int(rng.integers(2, 10))
        spans.append((pos, pos + n))
        pos += n + int(rng.integers(0, 6))
    case("gaps", 1500, spans, 60)
    # long spans: windows with too few labels (<= 2) and with too little signal (<= 0.3 * seq_length)
    spans = [(i * 40, i * 40 + 35) for i in range(12)]          # 11 guard spans -> skip_start
    spans += [(500, 540), (540, 580), (580, 620)]               # spans of 40: a window holds two of them (<= 2 labels) -> rejected
    spans += [(620, 630), (630, 640), (640, 645), (645, 740)]   # 25 samples, 3 labels: too little signal for 100
    spans += [(740 + 3 * i, 743 + 3 * i) for i in range(40)]
    spans += [(900, 1050)]                                      # a span longer than the window
    spans += [(1050 + 7 * i, 1057 + 7 * i) for i in range(30)]
    spans += [(1300 + i * 5, 1305 + i * 5) for i in range(12)]  # tail guard
    case("rejections", 1400, spans, 100)
    # the last kept window is padded from a signal that ends within seq_length: short padding
    pos, spans = 0, []
    while pos < 585:
        spans.append((pos, pos + 6))
        pos += 6
    case("short_padding", 600, spans, 80)
    # the span that closes the last kept window ends 5 samples before the signal does: its padding is 4 samples of signal
    # (the reference keeps spans that end strictly before the end) and zeros after them
    spans = [(3 * i, 3 * i + 3) for i in range(10)]                       # head guard
    spans += [(30 + 6 * i, 36 + 6 * i) for i in range(8)]                 # 48 samples, 8 labels
    spans += [(78, 95)]                                                   # does not fit in 60: closes the window, 95 + 4 < 100
    spans += [(95 + i // 10, 95 + i // 10 + 1) for i in range(10)]        # tail guard (skip_start), inside the signal
    case("zero_fill", 100, spans, 60)
    return cases


def main():
    from make_golden import import_reference
    chiron_input, _, _ = import_reference()
    import tempfile
    out = []
    for c in make_cases():
        with tempfile.TemporaryDirectory() as d:
            lf = os.path.join(d, "x.label")
            with open(lf, "w") as f:
                f.write("\n".join(c["label_lines"]) + "\n")
            lab = chiron_input.read_label(lf, skip_start=10, window_n=0)
            sig = [float(np.float32(v)) for v in c["signal"]]
            ev, el, lb, ll = chiron_input.read_raw(sig, lab, c["seq_length"])
        out.append(dict(c, raw_label={"start": [int(v) for v in lab.start], "length": [int(v) for v in lab.length],
                                      "base": [int(v) for v in lab.base]},
                        event=[[float(v) for v in e] for e in ev], event_length=[int(v) for v in el],
                        label=[[int(v) for v in x] for x in lb], label_length=[int(v) for v in ll]))
    with open(os.path.join(HERE, "labelled_windows.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    for c in out:
        print(c["name"], "windows", len(c["event"]), "labels", c["label_length"])


if __name__ == "__main__":
    main()
