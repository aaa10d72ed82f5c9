#!/usr/bin/env python
"""Time chiron_event_locate (csrc/event_locate.hip) against chiron_signal_locate (csrc/locate.hip) on the same queries in the same
run: tools/bench_locate.py's workload -- 2048 walks of 2000 samples at a geometric dwell of mean 9 with noise of sd 3 x 25.6 int16
units on both strands of a random 50 kb genome under a random 5-mer table, 100,001 columns.  The samples are cut into events once,
by one chiron_signal_events call at the defaults of `locate --events` (timed on its own, outside the rounds).  Then the rounds
alternate -- a chiron_signal_locate call on the samples, a chiron_event_locate call on the events -- and the medians of --rounds
rounds after a warm-up are taken.  Each is a whole library call on prepared arrays: the host's checking walk, the copies in, the
launches, the copy out.  As context the numpy rows of tests/event_ref.py run on one core over the first --ref-queries queries' events,
scaled to the whole by cells; their triples must equal the library's or the tool exits non-zero.  The result goes to
profiles/event_locate.json: both times, the cells a second of each, the events a query, the share of queries that end within 3 and
within 32 columns of the walk's last column for both, and the margins.

The one performance condition is checked here: the event call must be faster than the sample call, a ratio above 1, or the tool
exits non-zero.  --library-only times nothing and runs the event call --rounds times: the form to put behind `rocprofv3
--kernel-trace --stats`.  Needs a GPU: there is nothing to time without one."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--genome", type=int, default=50000)
    ap.add_argument("--dwell", type=float, default=9.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--ref-queries", dest="ref_queries", type=int, default=1, help="queries the numpy reference runs on; its time is scaled by cells")
    ap.add_argument("--library-only", dest="library_only", action="store_true", help="only run the event call --rounds times, write nothing")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "event_locate.json"))
    args = ap.parse_args()
    import torch
    from chiron_amd import _lib, locate
    import event_ref as ref
    from bench_locate import make_case
    if not torch.cuda.is_available():
        sys.exit("bench_event_locate: no GPU")
    rng = np.random.default_rng(20261020)
    row, cmap, x, true_end = make_case(rng, args.genome, args.queries, args.samples, args.dwell)
    items, ref_len = args.queries, len(row)
    samples = np.ascontiguousarray(x.reshape(-1))
    sample_off = np.arange(items + 1, dtype=np.int64) * args.samples
    d = locate.EVENT_DEFAULTS
    penalty, thr = d["penalty"], locate.event_threshold(d["threshold"])
    lib = _lib.load()

    # the events, once
    count, cut = np.zeros(items, np.int32), np.zeros(items, np.uint8)
    border, level = np.zeros(len(samples) + items, np.int32), np.zeros(len(samples), np.int16)
    t0 = time.perf_counter()
    _lib.check(lib.chiron_signal_events(samples.ctypes.data, sample_off.ctypes.data, items, d["window"], d["radius"], thr, locate.EVENT_MAX_QUERY, 0,
                                        count.ctypes.data, border.ctypes.data, level.ctypes.data, cut.ctypes.data))
    segment_ms = (time.perf_counter() - t0) * 1e3
    queries = [level[i * args.samples:i * args.samples + int(count[i])] for i in range(items)]
    events = np.ascontiguousarray(np.concatenate(queries + [np.zeros(1, np.int16)]))
    event_off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    n_events = int(event_off[-1])

    need_s = locate.workspace_size(items, items * args.samples, ref_len)
    need_e = locate.workspace_size_events(items, n_events, ref_len)
    lib, ws, stream = _lib.device_workspace(max(need_s, need_e), 0, "bench_event_locate", "locate kernels")     # one after the other: one workspace
    blocks = locate.blocks_of_ref(ref_len)
    out_s, out_e = np.zeros((items, blocks, 3), dtype=np.int32), np.zeros((items, blocks, 3), dtype=np.int32)

    def call_samples():
        _lib.check(lib.chiron_signal_locate(0, samples.ctypes.data, sample_off.ctypes.data, items, row.ctypes.data, ref_len, out_s.ctypes.data, ws.data_ptr(),
                                            need_s, 0, stream))

    def call_events():
        _lib.check(lib.chiron_event_locate(0, events.ctypes.data, event_off.ctypes.data, items, row.ctypes.data, ref_len, penalty, out_e.ctypes.data,
                                           ws.data_ptr(), need_e, 0, stream))

    launches = (int(count.max()) + _lib.EVENT_CHUNK - 1) // _lib.EVENT_CHUNK
    if args.library_only:
        for _ in range(args.rounds):
            call_events()
        print("bench_event_locate: %d calls of %d queries of %.1f events on %d columns, %d launches each" % (args.rounds, items, n_events / items, ref_len, launches))
        return
    torch.set_num_threads(1)
    for _ in range(args.warmup):
        call_samples()
        call_events()
    sub = min(args.ref_queries, items)
    sample_ms, event_ms, numpy_sub_ms = [], [], []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        call_samples()
        sample_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        call_events()
        event_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        want = ref.locate(queries[:sub], row, penalty)
        numpy_sub_ms.append((time.perf_counter() - t0) * 1e3)
        if not np.array_equal(out_e[:sub], want):
            sys.exit("bench_event_locate: the library call and the numpy reference differ on the first %d queries" % sub)
    med = lambda v: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}

    def accuracy(out, spans, per):
        summary = [locate.summarise(b, int(n)) for b, n in zip(out, spans)]
        err = np.array([abs(s["best"][1] - t) for s, t in zip(summary, true_end)])
        margins = np.array([(s["second"] - s["best"][0]) / float(p) for s, p in zip(summary, per) if s["second"] is not None])
        return {"ends_within_3_columns": float((err <= 3).mean()), "ends_within_32_columns": float((err <= 32).mean()),
                "margin": med(margins) if len(margins) else None, "queries_with_margin": int(len(margins))}
    cells_s, cells_e = items * args.samples * ref_len, n_events * ref_len
    ratio = float(np.median(sample_ms)) / float(np.median(event_ms))
    numpy_ms = float(np.median(numpy_sub_ms)) * n_events / int(event_off[sub])
    result = {"device": torch.cuda.get_device_name(0), "queries": items, "samples_per_query": args.samples, "genome": args.genome, "columns": ref_len,
              "mean_dwell": args.dwell, "rounds": args.rounds, "detector": {"window": d["window"], "threshold_int": thr, "radius": d["radius"]},
              "skip_penalty": penalty, "segment_ms": segment_ms, "events_per_query": med(count), "samples_per_event": len(samples) / n_events,
              "truncated": int(cut.sum()), "event_launches": launches,
              "samples": dict(call_ms=med(sample_ms), cells=cells_s, cells_per_second=cells_s / (float(np.median(sample_ms)) * 1e-3),
                              workspace_bytes=int(need_s), margin_unit="per sample", **accuracy(out_s, [args.samples] * items, [args.samples] * items)),
              "events": dict(call_ms=med(event_ms), cells=cells_e, cells_per_second=cells_e / (float(np.median(event_ms)) * 1e-3),
                             workspace_bytes=int(need_e), margin_unit="per event", **accuracy(out_e, 2 * count, count)),
              "sample_call_over_event_call": ratio, "numpy_queries": sub, "numpy_subset_ms": med(numpy_sub_ms), "numpy_ms_scaled": numpy_ms,
              "numpy_over_event_call": numpy_ms / float(np.median(event_ms)),
              "note": "each call_ms is a whole library call on prepared arrays; segment_ms is the one chiron_signal_events call that made the events and "
                      "is in neither; numpy_ms_scaled is tests/event_ref.py's numpy rows on one core over numpy_queries queries, scaled to all by cells"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
    print(json.dumps(result))
    if not ratio > 1.0:
        sys.exit("bench_event_locate: the event call is not faster than the sample call on the same queries")


if __name__ == "__main__":
    main()
