"""Command line (counterpart of chiron/entry.py): `python -m chiron_amd.entry call ...`.

Keeps the reference's `chiron call` flags and presets (entry.py:19-47, :69-92); only inference is
built (export/train are out of scope)."""
import argparse
import sys
from os import path

from . import __version__
from .map import DEFAULT_SEED


def set_paras(args, p):
    """entry.py:53-60: explicit flags win over the preset."""
    args.start = p["start"] if args.start is None else args.start
    args.batch_size = p["batch_size"] if args.batch_size is None else args.batch_size
    args.segment_len = p["segment_len"] if args.segment_len is None else args.segment_len
    args.jump = p["jump"] if args.jump is None else args.jump
    args.threads = p["threads"] if args.threads is None else args.threads
    args.beam = p["beam"] if args.beam is None else args.beam
    return args


def resolve_preset(args):
    """entry.py:20-32."""
    if args.preset is None:
        default_p = {"start": 0, "batch_size": 400, "segment_len": 500, "jump": 490, "threads": 0, "beam": 30}
    elif args.preset == "dna-pre":
        default_p = {"start": 0, "batch_size": 400, "segment_len": 400, "jump": 390, "threads": 0, "beam": 30}
        if args.mode == "rna":
            raise ValueError("Try to use the DNA preset parameter setting in RNA mode.")
    elif args.preset == "rna-pre":
        default_p = {"start": 0, "batch_size": 300, "segment_len": 2000, "jump": 1900, "threads": 0, "beam": 30}
        if args.mode == "dna":
            raise ValueError("Attempt to use the RNA preset parameter setting in DNA mode, enable RNA basecalling by --mode rna")
    else:
        raise ValueError("Unknown presetting %s undifiend" % (args.preset))
    return set_paras(args, default_p)


def evaluation(args):
    """entry.py:19-47: extract fast5 -> <out>/raw, then basecall <out>/raw."""
    import os as _os
    n_gpus = int(getattr(args, "gpus", 0) or 0)
    child_vars = [v for v in ("CHIRON_LOCAL_RANK", "CHIRON_LOCAL_WORLD", "CHIRON_BARRIER_DIR") if _os.environ.get(v)]
    if child_vars and len(child_vars) != 3:
        # a rank of `chiron call --gpus N` gets all three from its parent; one or two of them is a stale export, and treating
        # the process as a rank would die later with a KeyError (or, worse, skip the spawn silently)
        raise RuntimeError("%s set without the other CHIRON_LOCAL_* variables: unset it (only `chiron call --gpus N` sets them, "
                           "all three, for its own ranks)" % ", ".join(child_vars))
    if n_gpus > 1 and not child_vars:
        # `chiron call --gpus N`: this process only starts the N ranks (one per GPU, each on its own slice of the host's cores)
        # and waits; the ranks shard the reads, meet at a file barrier and rank 0 gathers merged.<ext> (shard.py)
        from . import shard
        resolve_preset(args)                       # a bad preset / mode fails here, once, not N times
        _os.makedirs(args.output, exist_ok=True)
        child_argv = getattr(args, "child_argv", None)
        if child_argv is None:
            # evaluation(args) called with a Namespace instead of through main(): the ranks need a command line
            raise ValueError("--gpus %d needs the command line to give its ranks: call chiron_amd.entry.main([...]) or set "
                             "args.child_argv" % n_gpus)
        codes = shard.spawn_local_ranks(child_argv, n_gpus, args.output, share_gpu=_os.environ.get("CHIRON_SHARE_GPU") == "1")
        if any(codes):
            raise RuntimeError("chiron call --gpus %d: rank exit codes %s" % (n_gpus, codes))
        return codes
    from . import eval as chiron_eval
    from .extract import extract
    args = resolve_preset(args)
    FLAGS = args
    FLAGS.input_dir = FLAGS.input
    FLAGS.output_dir = FLAGS.output
    FLAGS.unit = False
    FLAGS.recursive = True
    FLAGS.polya = None
    FLAGS.idname = False
    FLAGS.delimiter = "\n"
    args.reverse_fast5 = args.mode == "rna"
    # One process per GPU (torchrun / torch.distributed.run): reads shard per rank -- extraction, basecalling and the
    # result files -- and are gathered on the host; no collective on the data path.
    from . import shard
    dist, rank, world, device = shard.init_distributed()
    if device is not None:
        FLAGS.device = device
    if path.isdir(FLAGS.input):
        from .extract import list_fast5, prepare_folders
        fast5_list = list_fast5(FLAGS.input, True, getattr(FLAGS, "test_number", None))
        if getattr(FLAGS, "via_signal_files", False):
            FLAGS.no_raw = False                          # the two-pass path reads raw/<name>.signal back: it must exist
        if fast5_list and not getattr(FLAGS, "via_signal_files", False):
            # Direct path: ONE partition decides which rank decodes and basecalls a fast5 file; the reader
            # threads write raw/<name>.signal for the output tree and window the decoded samples straight away -- no
            # extract-everything barrier, no text parsed back.
            import os
            from .extract import unique_read_files, logger
            prepare_folders(FLAGS, rank, world)
            fast5_list, dropped = unique_read_files(fast5_list)       # before partitioning: every rank drops the same files
            for lost, kept in (dropped if rank == 0 else []):
                logger.error("Read name of %s is taken by %s as well: the reference's extraction would overwrite the first; only the "
                             "second is basecalled." % (lost, kept))
            FLAGS.input = FLAGS.output + "/raw/"          # what the .meta files record (entry.py:38)
            sizes = {f: os.path.getsize(f) for f in fast5_list}
            FLAGS.fast5_files = shard.partition_reads(fast5_list, world, rank, sizes)
            if dist is None:
                return chiron_eval.run(args)
            out = shard.run_sharded(FLAGS, lambda fl, mine: chiron_eval.evaluation(fl, fast5_files=fl.fast5_files), dist,
                                    partition=False)
            dist.destroy_process_group()
            return out
        if fast5_list:
            # the reference's own two passes (entry.py:33-38): extract every file to raw/*.signal, then basecall raw/
            extract(FLAGS, rank, world)
            if dist is not None:
                dist.barrier()
            FLAGS.input = FLAGS.output + "/raw/"
        # else: a folder of .signal files (what extraction would have produced) is basecalled in place
    if dist is None:
        return chiron_eval.run(args)
    out = shard.run_sharded(FLAGS, lambda fl, mine: chiron_eval.evaluation(fl, file_list=mine), dist)
    dist.destroy_process_group()
    return out


def validate(args):
    """Score a model on labelled windows, as the reference's training loop validates (chiron_model.loss, chiron_model.py:50-75, and
    prediction, :101-132): windows from a folder of .signal + .label pairs (labelled.py, chiron_input.py:429-525), the engine's
    logits and decode, then per row the CTC loss and the normalized edit distance on the GPU (Engine.score).  seq_len is what
    `chiron call` feeds (seq_len_for_engine: round half even of len / ratio, chiron_eval.py:337); the reference's training loop
    truncates len / ratio instead, which differs only where the ratio does not divide the length (RNA, ratio 5).  Writes a JSON
    report to args.output and returns it."""
    import json
    import numpy as np
    from . import ctc, labelled, model as model_mod
    from .engine import Engine, seq_len_for_engine
    ds = labelled.read_raw_data_sets(args.input, seq_length=args.segment_len, max_segments=args.max_segments, sig_norm=args.sig_norm)
    n = ds.event.shape[0]
    if n == 0:
        raise ValueError("no labelled window under %s" % args.input)
    spec, weights, _ = model_mod.load_model(args.model, allow_synthetic=args.synthetic_weights)
    batches, losses, edits, stats = [], [], [], []
    with Engine(spec, weights, max_batch=min(args.batch_size, n), segment_len=args.segment_len, device_id=args.device,
                max_beam=args.beam, dtype=args.dtype, calibrate=not args.no_calibration) as eng:
        for i in range(0, n, args.batch_size):
            x = np.ascontiguousarray(ds.event[i:i + args.batch_size], dtype=np.float32)
            sl = seq_len_for_engine(ds.event_length[i:i + args.batch_size], eng.ratio)
            ll = ds.label_length[i:i + args.batch_size]
            dense = labelled.dense_labels(ds.label[i:i + args.batch_size], ll)
            eng.submit(0, x, sl, beam_width=args.beam, want_prob=False)
            eng.collect(0)
            loss, edit, status = eng.score(0, dense, ll)
            losses.append(loss)
            edits.append(edit)
            stats.append(status)
            kept = status != ctc.STATUS_INFEASIBLE
            batches.append({"loss_mean": float(np.mean(np.where(kept, loss, 0.0)[kept], dtype=np.float64)) if kept.any() else None,
                            "error_mean": float(np.mean(edit, dtype=np.float64)), "n": int(x.shape[0]),
                            "skipped": int(np.count_nonzero(status == ctc.STATUS_SKIPPED)),
                            "infeasible": int(np.count_nonzero(status == ctc.STATUS_INFEASIBLE))})
    loss = np.concatenate(losses)
    edit = np.concatenate(edits)
    status = np.concatenate(stats)
    kept = status != ctc.STATUS_INFEASIBLE
    summary = {"windows": int(n), "files": len(set(ds.files)),
               # tf.reduce_mean of the per-row losses: skipped rows count as 0 (their loss is 0), infeasible rows -- where TF raises --
               # are left out and counted
               "loss_mean_reference": float(np.mean(loss[kept], dtype=np.float64)) if kept.any() else None,
               "skipped": int(np.count_nonzero(status == ctc.STATUS_SKIPPED)), "infeasible": int(np.count_nonzero(~kept)),
               "error_mean": float(np.mean(edit, dtype=np.float64))}
    if args.fl_gamma > 0:
        summary["fl_gamma"] = args.fl_gamma
        summary["focal_loss_mean_reference"] = float(np.mean(ctc.focal(loss[kept], args.fl_gamma))) if kept.any() else None
    report = {"model": args.model, "input": args.input, "segment_len": args.segment_len, "batch_size": args.batch_size,
              "beam": args.beam, "dtype": args.dtype, "sig_norm": args.sig_norm, "batches": batches, "summary": summary}
    with open(args.output, "w") as f:
        json.dump(report, f, indent=1)
    return report


def finetune(args):
    """Adapt the recurrent stack and the FC head of a model to labelled reads, the CNN frozen: train.finetune (the loop of
    chiron_rcnn_train.py:99-135 on the GPU)."""
    import logging
    from . import train
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    return train.finetune(args)


def train(args):
    """Train every variable of the network on labelled reads: train.train_network (the loop of chiron_rcnn_train.py:99-135 on the GPU)."""
    import logging
    from . import train as train_mod
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    return train_mod.train_network(args)


def assess(args):
    """Read-level accuracy of called reads against per-read references: assess.assess (global alignment on the GPU, identity,
    mismatch, insertion and deletion rates).  Writes a JSON report to args.output; exits non-zero when no read found its
    reference."""
    import json
    from . import assess as assess_mod
    if getattr(args, "genome", None):             # no per-read references: map against the genome first (map.py)
        from . import map as map_mod
        if args.reference:
            raise ValueError("assess: give the references with -r or a genome with -g, not both")
        report = map_mod.assess_genome(args.input, args.genome, workspace_mb=args.workspace_mb, device_id=args.device, profile=args.profile,
                                       seed=getattr(args, "seed", DEFAULT_SEED), candidates=getattr(args, "candidates", 1),
                                       second_ratio=getattr(args, "second_ratio", 0.5))
    else:
        report = assess_mod.assess(args.input, args.reference, strand=args.strand, device_id=args.device, profile=args.profile,
                                   workspace_mb=args.workspace_mb)
    with open(args.output, "w") as f:
        json.dump(report, f, indent=1)
    pooled = report["pooled"]
    print("assess: %d reads paired, %d unpaired; pooled identity %.4f, mismatch %.4f, insertion %.4f, deletion %.4f"
          % (report["paired"], report["unpaired_count"], pooled["identity"], pooled["mismatch_rate"], pooled["insertion_rate"],
             pooled["deletion_rate"]))
    for name in report["unpaired"]:
        print("assess: no reference for read %s" % name, file=sys.stderr)
    if report["paired"] == 0:
        sys.exit("assess: no read under %s found its reference under %s" % (report["input"], report["reference"] or args.genome))
    return report


def overlap(args):
    """Read-to-read overlaps without a genome: overlap.overlap_command (k-mer votes of every read against the later ones on the
    host, exact banded dovetail alignment of every candidate pair on the GPU).  Writes <out>/overlaps.paf and
    <out>/overlap_report.json."""
    from . import overlap as overlap_mod
    report = overlap_mod.overlap_command(args.input, args.output, min_votes=args.min_votes, max_occ=args.max_occ, max_overlaps=args.max_overlaps,
                                         band=args.band, min_overlap=args.min_overlap, min_identity=args.min_identity,
                                         workspace_mb=args.workspace_mb, device_id=args.device)
    print("overlap: %d reads, %d candidate pairs; %d overlaps kept (%s); dropped: %d short, %d below the identity, %d at a band edge"
          % (report["reads"], report["candidate_pairs"], report["kept"]["total"],
             ", ".join("%d %s" % (report["kept"][t], t) for t in overlap_mod.TYPES), report["dropped"]["short"], report["dropped"]["identity"],
             report["edge"]))
    return report


def map_reads(args):
    """Place called reads in a genome: map.map_command (k-mer votes and exact infix alignment, both on the GPU).  Writes
    <out>/reference/<read>_ref.fasta (what `assess -r` and `label -r` take), <out>/mapped.paf and <out>/map_report.json; exits
    non-zero when no read mapped."""
    from . import map as map_mod
    report = map_mod.map_command(args.input, args.genome, args.output, min_votes=args.min_votes, max_occ=args.max_occ, band=args.band,
                                 workspace_mb=args.workspace_mb, device_id=args.device, cigar=args.cigar, seed=getattr(args, "seed", DEFAULT_SEED),
                                 candidates=getattr(args, "candidates", 1), second_ratio=getattr(args, "second_ratio", 0.5))
    t = report["totals"]
    print("map: %d reads; %d mapped, %d unmapped, %d at a window edge; identity of the mapped reads %.4f"
          % (t["reads"], t["mapped"], t["unmapped"], t["edge"], t["identity"]))
    if "mapq0" in report:
        print("map: up to %d candidates a read; mapq 0: %d reads, 1 .. 59: %d, 60: %d; %d won by a pick other than the first"
              % (report["candidates"], report["mapq0"], report["mapq1_59"], report["mapq60"], report["won_by_later_pick"]))
    for name in report["unmapped"]:
        print("map: read %s did not map" % name, file=sys.stderr)
    if t["mapped"] == 0:
        sys.exit("map: no read under %s mapped to %s" % (args.input, args.genome))
    return report


def pileup(args):
    """Consensus and variants from mapped reads: pileup.pileup_command (the columns of every alignment summed per genome position and
    called on the GPU).  Writes <out>/consensus.fasta (a valid -r / -g for `assess` and `map`), <out>/variants.tsv and
    <out>/pileup_report.json; exits non-zero on an input without a mapped.sam or without a usable alignment."""
    from . import pileup as pileup_mod
    try:
        report = pileup_mod.pileup_command(args.input, args.genome, args.output, min_depth=args.min_depth, workspace_mb=args.workspace_mb,
                                           device_id=args.device, min_mapq=getattr(args, "min_mapq", 0))
    except ValueError as e:
        sys.exit("pileup: %s" % e)
    t = report["totals"]
    print("pileup: %d alignments over %d positions, mean depth %.2f; %d substitutions, %d deletions, %d insertions applied; %d positions "
          "below depth %d" % (report["alignments_used"], t["length"], t["mean_depth"], t["substitutions"], t["deletions"], t["insertions"],
                              t["low_depth"], report["min_depth"]))
    if report["alignments_used"] == 0:
        sys.exit("pileup: %s holds no usable alignment" % report["sam"])
    return report


def polish(args):
    """Rescore the pileup's candidate variants with the reads' CTC likelihoods: polish.polish_command (the frames of every read
    that covers a variant scored against both alleles on the GPU).  Writes <out>/polished.fasta (a valid -g for `map`, `assess` and
    `pileup`), <out>/polish_variants.tsv and <out>/polish_report.json; exits non-zero on an input without a mapped.sam or when no
    read could be used."""
    import logging
    from . import polish as polish_mod
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    try:
        report = polish_mod.polish_command(args)
    except ValueError as e:
        sys.exit("polish: %s" % e)
    print("polish: %d candidates, %d scored by %d of %d reads (%d read windows); %d eligible, %d accepted (%d substitutions, %d deletions, "
          "%d insertions)" % (report["candidates"]["total"], report["candidates"]["scored"], report["reads"]["used"], report["reads"]["total"],
                              report["items"]["scored"], report["eligible"], report["accepted"]["total"], report["accepted"]["SUB"],
                              report["accepted"]["DEL"], report["accepted"]["INS"]))
    if report["reads"]["used"] == 0:
        sys.exit("polish: no read of %s could be used (%s)" % (report["sam"], report["reads"]["dropped"]))
    return report


def label(args):
    """Labels from the model's own logits: label.label (CTC forced alignment of every read's frames to its reference bases on the
    GPU).  Writes <out>/<read>.signal + <out>/<read>.label, a folder `validate`, `finetune` and `train` take as -i, and
    <out>/label_report.json; exits non-zero when no read was labelled."""
    import logging
    from . import label as label_mod
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    if args.mode not in ("dna", "rna"):
        raise ValueError("--mode must be dna or rna, not %r" % (args.mode,))
    if getattr(args, "genome", None):             # no per-read references: cut them out of the genome first (map.py)
        from . import assess as assess_mod, map as map_mod
        if args.reference:
            raise ValueError("label: give the references with -r or a genome with -g, not both")
        seed = getattr(args, "seed", DEFAULT_SEED)
        mapped = map_mod.map_reads(assess_mod.load_reads(args.input), map_mod.load_genome(args.genome), device_id=args.device,
                                   seeder=map_mod.seeder_of(seed, device_id=args.device), candidates=getattr(args, "candidates", 1),
                                   second_ratio=getattr(args, "second_ratio", 0.5),
                                   top_seeder=map_mod.top_seeder_of(seed, device_id=args.device))
        args.reference = path.join(args.output, "reference")
        map_mod.write_references(args.reference, mapped["references"])
    report = label_mod.label(args)
    t = report["totals"]
    print("label: %d reads written; %d aligned, %d infeasible, %d band exhausted, %d skipped, %d without a reference"
          % (t["written"], t["aligned"], t["infeasible"], t["band_exhausted"], t["skipped"], report["no_reference_count"]))
    for name in report["no_reference"]:
        print("label: no reference for read %s" % name, file=sys.stderr)
    if t["written"] == 0:
        sys.exit("label: no read under %s was labelled" % args.input)
    return report


def demux(args):
    """Split called reads by barcode and trim their ends: demux.demux_command (every read end searched for every barcode on the GPU).
    Writes <out>/<barcode>.fastq per bin (each a valid -i of `map` and `assess`), <out>/unclassified.fastq, <out>/demux.tsv and
    <out>/demux_report.json; exits non-zero on an input without reads or a barcode file without usable records."""
    from . import demux as demux_mod
    try:
        report = demux_mod.demux_command(args.input, args.barcodes, args.output, window=args.window, max_err=args.max_err,
                                         min_margin=args.min_margin, require=args.require, do_trim=not args.no_trim,
                                         workspace_mb=args.workspace_mb, device_id=args.device)
    except ValueError as e:
        sys.exit("demux: %s" % e)
    s = report["status"]
    print("demux: %d reads against %d patterns; %d classified into %d bins, %d unclassified, %d in conflict, %d empty after trimming; "
          "%d of %d bases written" % (report["reads"], report["patterns"], s["classified"], sum(1 for v in report["bins"].values() if v),
                                      s["unclassified"], s["conflict"], s["empty"], report["bases"]["written"], report["bases"]["in"]))
    return report


def squiggle(args):
    """The reads' current levels on the genome: squiggle.squiggle_command (the samples of every called base reduced to a level and the
    levels summed per position and strand on the GPU).  Writes <out>/levels.tsv and <out>/squiggle_report.json, with --control
    <out>/compare.tsv (Welch's t per position against the control sample), with --kmer <out>/kmer_levels.tsv and with --events
    <out>/events/<read>.tsv; with --refine the base borders are first moved to where the samples meet a level table; exits non-zero on an input without a mapped.sam or when no read could be used."""
    import logging
    from . import squiggle as squiggle_mod
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    try:
        report = squiggle_mod.squiggle_command(args)
    except ValueError as e:
        sys.exit("squiggle: %s" % e)
    print("squiggle: %d of %d reads used, %d bases and %d samples in %d tiles; %d events on the genome; wrote %s"
          % (report["reads"]["used"], report["reads"]["total"], report["bases"], report["samples"], report["tiles"], report["events"],
             ", ".join(report["files"])))
    if report["reads"]["used"] == 0:
        sys.exit("squiggle: no read of %s could be used (%s)" % (report["sam"], report["reads"]["dropped"]))
    return report


def locate(args):
    """Where on the genome raw signal comes from, without calling it: locate.locate_command (the reads' first samples against the
    expected levels of both strands under a k-mer level table, by subsequence DTW on the GPU).  Writes <out>/located.tsv and
    <out>/locate_report.json; exits non-zero on a file that is no level table or when no read gave a query."""
    from . import locate as locate_mod
    try:
        report = locate_mod.locate_command(args)
    except ValueError as e:
        sys.exit("locate: %s" % e)
    s = report["status"]
    print("locate: %d of %d reads used against %d columns in %d calls; %d placed, %d ambiguous, %d unplaced; wrote %s"
          % (report["reads"]["used"], report["reads"]["total"], report["columns"], report["batches"], s["placed"], s["ambiguous"], s["unplaced"],
             ", ".join(report["files"])))
    if report["reads"]["used"] == 0:
        sys.exit("locate: no read of %s gave a query (%s)" % (report["signal"], report["reads"]["dropped"]))
    return report


def modcall(args):
    """Per-read calls of modified bases at motif sites: modcall.modcall_command (every read's samples around every motif group fitted
    to the window's levels under a canonical and under a modified k-mer level table, by an exact DTW on the GPU).  Writes
    <out>/mod_calls.tsv, <out>/mod_sites.tsv and <out>/modcall_report.json; exits non-zero on a file that is no level table, on two
    tables of different k, on an input without a mapped.sam or when no read could be used."""
    from . import modcall as modcall_mod
    try:
        report = modcall_mod.modcall_command(args)
    except ValueError as e:
        sys.exit("modcall: %s" % e)
    c = report["calls"]
    print("modcall: %d of %d reads used; %d of %d (read, group) pairs scored in %d calls; %d modified, %d canonical, %d ambiguous at %d sites; wrote %s"
          % (report["reads"]["used"], report["reads"]["total"], report["groups"]["scored"], report["groups"]["seen"], report["batches"], c["modified"],
             c["canonical"], c["ambiguous"], report["sites"], ", ".join(report["files"])))
    if report["reads"]["used"] == 0:
        sys.exit("modcall: no read of %s could be used (%s)" % (report["sam"], report["reads"]["dropped"]))
    return report


def build_parser():
    parser = argparse.ArgumentParser(prog="chiron", description="A deep neural network basecaller (MI355X engine).")
    parser.add_argument("-v", "--version", action="version", version="chiron_amd version " + __version__)
    subparsers = parser.add_subparsers(title="sub command", help="sub command help")
    model_default_path = path.join(path.abspath(path.dirname(__file__)), "model", "DNA_default")
    p = subparsers.add_parser("call", description="Perform basecalling", help="Perform basecalling.")
    p.add_argument("-i", "--input", required=True, help="File path or Folder path to the fast5 file.")
    p.add_argument("-o", "--output", required=True, help="Output folder path")
    p.add_argument("-m", "--model", type=str, default=model_default_path, help="model folder path")
    p.add_argument("-s", "--start", type=int, default=None, help="Start index of the signal file.")
    p.add_argument("-b", "--batch_size", type=int, default=None, help="Batch size for run.")
    p.add_argument("-l", "--segment_len", type=int, default=None, help="Segment length to be divided into.")
    p.add_argument("-j", "--jump", type=int, default=None, help="Step size for segment")
    p.add_argument("-t", "--threads", type=int, default=None, help="Host threads, 0 = all.")
    p.add_argument("--finish-procs", type=int, default=0,
                   help="Worker processes for consensus / quality / writers (0: threads; useful behind the fp16 engine).")
    p.add_argument("-e", "--extension", default="fastq", help="Output file type.")
    p.add_argument("--beam", type=int, default=None, help="Beam width of the CTC beam search decoder, 0 = greedy.")
    p.add_argument("--concise", action="store_true", help="Only write the result files.")
    p.add_argument("--mode", default="dna", help="Output mode, dna or rna.")
    p.add_argument("--test_number", default=None, type=int, help="Extract test_number reads, default all.")
    p.add_argument("-p", "--preset", default=None, help="Preset evaluation parameters: dna-pre, rna-pre")
    p.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    p.add_argument("--gpus", type=int, default=0,
                   help="Basecall on this many GPUs of the node: the command starts one process per GPU itself (reads sharded per "
                        "process, host-side gather into merged.<ext>, per-process CPU affinity); 0 / 1: this process, --device.  "
                        "(torch.distributed.run launches are honoured as before.)")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "fp16", "fp16-w2", "fp32-split"],
                   help="Engine arithmetic: fp32 (parity path), fp16 (f16 MFMA conv + LSTM, fp32 CTC), fp16-w2 (fp16's activations against "
                        "exact hi + lo weights: the f16 mode for trained checkpoints), fp32-split "
                        "(fp32 values as hi/lo half pairs on the f16 matrix cores).")
    p.add_argument("--no-raw", dest="no_raw", action="store_true",
                   help="fast5 input on the direct path: do not write raw/<name>.signal (the reference's extraction output, "
                        "extract_sig_ref.py:119-123 -- 4 bytes of text per sample that nothing reads back here).  Opt-in deviation from the "
                        "reference's output tree; ignored with --via-signal-files.")
    p.add_argument("--no-calibration", dest="no_calibration", action="store_true",
                   help="--dtype fp16: skip the bias correction for the weights' rounding to halves (Engine.calibrate on a fixed synthetic "
                        "calibration batch at start-up).")
    p.add_argument("--via-signal-files", dest="via_signal_files", action="store_true",
                   help="fast5 input: the reference's two passes (extract everything to raw/*.signal, then parse the text back) "
                        "instead of windowing the decoded samples directly; same output files.")
    p.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                   help="Use seeded synthetic weights when the model folder has no checkpoint data.")
    p.set_defaults(func=evaluation)
    v = subparsers.add_parser("validate", description="Score a model on labelled .signal/.label pairs: CTC loss and edit distance",
                              help="CTC loss and normalized edit distance against known bases.")
    v.add_argument("-i", "--input", required=True, help="Folder of .signal files with their .label files.")
    v.add_argument("-m", "--model", type=str, default=model_default_path, help="model folder path")
    v.add_argument("-o", "--output", required=True, help="JSON report path")
    v.add_argument("-l", "--segment_len", type=int, default=400, help="Window length (the reference's sequence_len).")
    v.add_argument("-b", "--batch_size", type=int, default=1100, help="Batch size.")
    v.add_argument("--beam", type=int, default=30, help="Beam width of the decoder for the edit distance, 0 = greedy.")
    v.add_argument("--sig_norm", default="none", choices=["none", "median", "mean"], help="Signal normalisation.")
    v.add_argument("--fl_gamma", type=float, default=0.0, help="Focal-loss gamma of the reported focal variant (0: none).")
    v.add_argument("--max_segments", type=int, default=None, help="Largest number of windows to read.")
    v.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    v.add_argument("--dtype", default="fp32", choices=["fp32", "fp16", "fp16-w2", "fp32-split"], help="Engine arithmetic.")
    v.add_argument("--no-calibration", dest="no_calibration", action="store_true", help="--dtype fp16: skip the bias correction.")
    v.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                   help="Use seeded synthetic weights when the model folder has no checkpoint data.")
    v.set_defaults(func=validate)
    t = subparsers.add_parser("finetune", description="Fine-tune the recurrent layers and the FC head on labelled .signal/.label pairs "
                              "(CNN frozen)", help="Fine-tune the recurrent layers and the head on labelled reads.")
    # names and defaults: chiron_rcnn_train.py:182-222
    t.add_argument("-i", "--input", required=True, help="Folder of .signal files with their .label files.")
    t.add_argument("-o", "--output", required=True, help="Folder the fine-tuned model is written to.")
    t.add_argument("-m", "--model", type=str, default=model_default_path, help="model folder to start from")
    t.add_argument("-v", "--validation", default=None, help="validation folder (default: the training windows)")
    t.add_argument("-s", "--sequence_len", type=int, default=400, help="the length of sequence")
    t.add_argument("-b", "--batch_size", type=int, default=300, help="Batch size")
    t.add_argument("-t", "--step_rate", type=float, default=4e-3, help="Step rate")
    t.add_argument("-x", "--max_steps", type=int, default=10000, help="Maximum step")
    t.add_argument("-n", "--segments_num", type=int, default=None, help="Maximum number of segments read into the training queue, default(None) read all.")
    t.add_argument("--gradient_clip", type=float, default=None, help="Clip every variable's gradient to this norm.")
    t.add_argument("--fl_gamma", type=float, default=0.0, help="Focal-loss gamma (0: plain CTC loss).")
    t.add_argument("--opt_method", default="Adam", choices=["Adam", "SGD", "RMSProp", "Momentum"], help="Optimizer.")
    t.add_argument("--sig_norm", default="none", choices=["none", "median", "mean"], help="Signal normalisation.")
    t.add_argument("--report-every", dest="report_every", type=int, default=10, help="Steps between loss / validation reports.")
    t.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    t.add_argument("--seed", type=int, default=1234, help="Seed of the batch order.")
    t.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                   help="Use seeded synthetic weights when the model folder has no checkpoint data.")
    t.set_defaults(func=finetune)
    r = subparsers.add_parser("train", description="Train the whole network (CNN, recurrent layers, FC head) on labelled .signal/.label pairs",
                              help="Train the whole network on labelled reads.")
    # names and defaults: chiron_rcnn_train.py:180-225
    r.add_argument("-i", "--input", required=True, help="Folder of .signal files with their .label files.")
    r.add_argument("-o", "--output", required=True, help="Folder the trained model is written to.")
    r.add_argument("-m", "--model", type=str, default=None, help="model folder to start from (default: a from-scratch initialisation)")
    r.add_argument("-v", "--validation", default=None, help="validation folder (default: the training windows)")
    r.add_argument("-s", "--sequence_len", type=int, default=400, help="the length of sequence")
    r.add_argument("-b", "--batch_size", type=int, default=300, help="Batch size")
    r.add_argument("-t", "--step_rate", type=float, default=4e-3, help="Step rate")
    r.add_argument("-x", "--max_steps", type=int, default=10000, help="Maximum step")
    r.add_argument("-n", "--segments_num", type=int, default=None, help="Maximum number of segments read into the training queue, default(None) read all.")
    r.add_argument("--configure", default=None, help="Model structure configure json file (a model.json) of a from-scratch model.")
    r.add_argument("--gradient_clip", type=float, default=None, help="Clip every variable's gradient to this norm.")
    r.add_argument("--retrain", dest="retrain", action="store_true", help="Continue from the newest checkpoint under -o.")
    r.add_argument("--bn", default="batch", choices=["population", "batch"],
                   help="BN naming of a from-scratch model: batch (HEAD's simple_global_bn, no statistics stored) or population.")
    r.add_argument("--fl_gamma", type=float, default=0.0, help="Focal-loss gamma (0: plain CTC loss).")
    r.add_argument("--opt_method", default="Adam", choices=["Adam", "SGD", "RMSProp", "Momentum"], help="Optimizer.")
    r.add_argument("--sig_norm", default="none", choices=["none", "median", "mean"], help="Signal normalisation.")
    r.add_argument("--report-every", dest="report_every", type=int, default=10, help="Steps between loss / validation reports.")
    r.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    r.add_argument("--seed", type=int, default=1234, help="Seed of the batch order and of the initialisation.")
    r.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                   help="Use seeded synthetic weights when the model folder has no checkpoint data.")
    r.set_defaults(func=train, retrain=False)
    a = subparsers.add_parser("assess", description="Read-level accuracy of called reads against per-read references: identity, "
                              "mismatch, insertion and deletion rates from a global alignment on the GPU",
                              help="Identity and error rates of called reads against their references.")
    a.add_argument("-i", "--input", required=True, help="Output folder of `call` (its result/ is read), or a fasta/fastq file or folder.")
    a.add_argument("-r", "--reference", default=None,
                   help="Folder of <read>_ref.fastq / <read>.fasta / <read>.fastq, or one fasta/fastq file with a record per read "
                        "(default: the reference/ folder of the `call` output).")
    a.add_argument("-g", "--genome", default=None,
                   help="A genome FASTA instead of -r: every read is mapped first (as `map` does) and assessed against the stretch it covers.")
    a.add_argument("-o", "--output", required=True, help="JSON report path")
    a.add_argument("--strand", default="forward", choices=["forward", "both"],
                   help="both: also align against the reverse complement of the reference and keep the better strand.")
    a.add_argument("--profile", action="store_true",
                   help="Also trace every pair on the GPU: the report gains each read's CIGAR (over =XID) and the pooled error profile "
                        "(substitution, insertion, deletion and homopolymer tables).")
    a.add_argument("--seed", default=DEFAULT_SEED, choices=["gpu", "host"],
                   help="Where the k-mer votes of the mapping are counted: on the GPU, or per read in numpy on the host (the reference; "
                        "the results are the same).")
    a.add_argument("--candidates", type=int, default=1,
                    help="Seeding candidates a read (1 to 8).  Above 1 the best candidates are all aligned, the best alignment wins and "
                         "the read gets a mapping quality (an ordering, not a calibrated probability; not tuned on real reads).")
    a.add_argument("--second-ratio", dest="second_ratio", type=float, default=0.5,
                    help="With --candidates above 1: a candidate is aligned when it has at least this share of the best one's votes "
                         "(not tuned on real reads).")
    a.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one traceback batch, MiB.")
    a.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    a.set_defaults(func=assess)
    lb = subparsers.add_parser("label", description="Make training labels: CTC forced alignment of each read's frame logits to its "
                               "reference bases on the GPU, written as .signal + .label pairs",
                               help="Write .signal/.label training pairs from reads and their references.")
    lb.add_argument("-i", "--input", required=True, help="Output folder of `call` (its raw/ and reference/ are read), or a folder of .signal files.")
    lb.add_argument("-r", "--reference", default=None,
                    help="Folder of <read>_ref.fastq / <read>.fasta / <read>.fastq, or one fasta/fastq file with a record per read "
                         "(default: the reference/ folder of the `call` output).")
    lb.add_argument("-g", "--genome", default=None,
                    help="A genome FASTA instead of -r: the called reads of -i (its result/) are mapped first (as `map` does) and the "
                         "stretches they cover are written to <output>/reference/ and used as the references.")
    lb.add_argument("--seed", default=DEFAULT_SEED, choices=["gpu", "host"],
                    help="Where the k-mer votes of the mapping are counted: on the GPU, or per read in numpy on the host (the reference; "
                         "the results are the same).")
    lb.add_argument("--candidates", type=int, default=1,
                    help="Seeding candidates a read (1 to 8).  Above 1 the best candidates are all aligned, the best alignment wins and "
                         "the read gets a mapping quality (an ordering, not a calibrated probability; not tuned on real reads).")
    lb.add_argument("--second-ratio", dest="second_ratio", type=float, default=0.5,
                    help="With --candidates above 1: a candidate is aligned when it has at least this share of the best one's votes "
                         "(not tuned on real reads).")
    lb.add_argument("-o", "--output", required=True, help="Folder the .signal/.label pairs and label_report.json are written to.")
    lb.add_argument("-m", "--model", type=str, default=model_default_path, help="model folder path")
    lb.add_argument("-l", "--segment_len", type=int, default=400, help="Window length; the windows do not overlap.")
    lb.add_argument("-b", "--batch_size", type=int, default=1100, help="Windows per engine batch.")
    lb.add_argument("--band", type=int, default=256, help="First half-width of the alignment band, in CTC states; 0: the full table (exact).")
    lb.add_argument("--max-band", dest="max_band", type=int, default=8192,
                    help="Largest half-width the doubling may reach before a read is given up (0: unbounded).")
    lb.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one alignment batch, MiB.")
    lb.add_argument("--mode", default="dna", help="dna or rna, as for `call` (U in a reference reads as T in either).")
    lb.add_argument("--dtype", default="fp32", choices=["fp32", "fp16", "fp16-w2", "fp32-split"], help="Engine arithmetic.")
    lb.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    lb.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                    help="Use seeded synthetic weights when the model folder has no checkpoint data.")
    lb.set_defaults(func=label)
    mp = subparsers.add_parser("map", description="Place called reads in a genome: k-mer votes, then exact infix alignment of "
                               "each read against its candidate window on the GPU",
                               help="Map called reads to a genome and cut out the per-read references.")
    mp.add_argument("-i", "--input", required=True, help="Output folder of `call` (its result/ is read), or a fasta/fastq file or folder.")
    mp.add_argument("-g", "--genome", required=True, help="Genome FASTA, one or many contigs.")
    mp.add_argument("-o", "--output", required=True, help="Folder reference/<read>_ref.fasta, mapped.paf and map_report.json are written to.")
    mp.add_argument("--min-votes", dest="min_votes", type=int, default=4, help="Fewest seed votes a read needs to be aligned at all.")
    mp.add_argument("--max-occ", dest="max_occ", type=int, default=64, help="K-mers that occur more often in the genome are not indexed.")
    mp.add_argument("--band", type=int, default=256, help="First half-width of the alignment band, in diagonals; 0: the full table.")
    mp.add_argument("--seed", default=DEFAULT_SEED, choices=["gpu", "host"],
                    help="Where the k-mer votes of the mapping are counted: on the GPU, or per read in numpy on the host (the reference; "
                         "the results are the same).")
    mp.add_argument("--candidates", type=int, default=1,
                    help="Seeding candidates a read (1 to 8).  Above 1 the best candidates are all aligned, the best alignment wins and "
                         "the read gets a mapping quality (an ordering, not a calibrated probability; not tuned on real reads).")
    mp.add_argument("--second-ratio", dest="second_ratio", type=float, default=0.5,
                    help="With --candidates above 1: a candidate is aligned when it has at least this share of the best one's votes "
                         "(not tuned on real reads).")
    mp.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one seeding or alignment batch, MiB.")
    mp.add_argument("--cigar", action="store_true",
                    help="Also trace every mapped read against the stretch it covers, in genome orientation: mapped.paf gains a cg:Z: "
                         "tag and mapped.sam is written.")
    mp.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    mp.set_defaults(func=map_reads)
    ov = subparsers.add_parser("overlap", description="Read-to-read overlaps without a genome: every read votes with its k-mers against the "
                               "later reads, and every candidate pair is aligned on the GPU by an exact banded dovetail alignment (a suffix "
                               "of one read against a prefix of the other, containment included).  The defaults are not tuned on real reads.",
                               help="All-against-all overlaps of called reads: overlaps.paf and a report.")
    ov.add_argument("-i", "--input", required=True, help="Output folder of `call` (its result/ is read), or a fasta/fastq file or folder.")
    ov.add_argument("-o", "--output", required=True, help="Folder overlaps.paf and overlap_report.json are written to.")
    ov.add_argument("--min-votes", dest="min_votes", type=int, default=4, help="Fewest seed votes a pair of reads needs to be aligned at all.")
    ov.add_argument("--max-occ", dest="max_occ", type=int, default=64, help="K-mers that occur more often in the reads are not indexed.")
    ov.add_argument("--max-overlaps", dest="max_overlaps", type=int, default=128,
                    help="Most candidates a read keeps against the reads after it, the highest votes first.")
    ov.add_argument("--band", type=int, default=256,
                    help="Half-width of the alignment band around the seeded diagonal.  The band is part of the result's definition: an "
                         "overlap on a diagonal outside it is not seen; a result on a band edge doubles the band, at most three times.")
    ov.add_argument("--min-overlap", dest="min_overlap", type=int, default=500, help="Shortest overlap that is kept, in bases of the shorter span.")
    ov.add_argument("--min-identity", dest="min_identity", type=float, default=0.7, help="Lowest identity M / (M + E) that is kept.")
    ov.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one alignment call, MiB.")
    ov.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    ov.set_defaults(func=overlap)
    pu = subparsers.add_parser("pileup", description="Consensus and variants from mapped reads: the alignment columns of mapped.sam summed "
                               "per genome position and called on the GPU",
                               help="Pile mapped reads up on the genome: consensus sequence, variants, report.")
    pu.add_argument("-i", "--input", required=True, help="Output folder of `map --cigar` (its mapped.sam is read), or a SAM file.")
    pu.add_argument("-g", "--genome", required=True, help="The genome FASTA the reads were mapped to.")
    pu.add_argument("-o", "--output", required=True, help="Folder consensus.fasta, variants.tsv and pileup_report.json are written to.")
    pu.add_argument("--min-depth", dest="min_depth", type=int, default=3, help="Positions covered by fewer alignments keep the genome's base.")
    pu.add_argument("--min-mapq", dest="min_mapq", type=int, default=0,
                    help="Drop alignments whose MAPQ is below this (`map --candidates` writes one; 255, not available, always passes).")
    pu.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one genome tile, MiB.")
    pu.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    pu.set_defaults(func=pileup)
    po = subparsers.add_parser("polish", description="Rescore the pileup's candidate variants with the reads' CTC likelihoods: the frames "
                               "of every read that covers a variant scored against both alleles on the GPU",
                               help="Polish a genome with the reads' frame scores: polished sequence, scored variants, report.")
    po.add_argument("-i", "--input", required=True, help="Output folder of `map --cigar` (its mapped.sam is read), or a SAM file.")
    po.add_argument("-s", "--signal", required=True, help="Output folder of `call` (its raw/ is read), or a folder of .signal files.")
    po.add_argument("-g", "--genome", required=True, help="The genome FASTA the reads were mapped to.")
    po.add_argument("-m", "--model", type=str, default=model_default_path, help="model folder path")
    po.add_argument("-o", "--output", required=True, help="Folder polished.fasta, polish_variants.tsv and polish_report.json are written to.")
    po.add_argument("--flank", type=int, default=8, help="Reference bases on either side of a variant in the scored window.")
    po.add_argument("--min-alt", dest="min_alt", type=int, default=2, help="Fewest reads that must show a variant for it to be a candidate.")
    po.add_argument("--min-frac", dest="min_frac", type=float, default=0.2, help="Smallest share of the depth that must show it.")
    po.add_argument("--min-llr", dest="min_llr", type=float, default=0.0,
                    help="A variant is eligible when its summed log-likelihood ratio exceeds this (not tuned on real reads).")
    po.add_argument("--min-reads", dest="min_reads", type=int, default=3, help="Fewest reads that must have scored a variant.")
    po.add_argument("--min-depth", dest="min_depth", type=int, default=3, help="As for `pileup`: the vote's own depth floor (reported only).")
    po.add_argument("--min-mapq", dest="min_mapq", type=int, default=0,
                    help="Drop alignments whose MAPQ is below this (`map --candidates` writes one; 255, not available, always passes).")
    po.add_argument("-l", "--segment_len", type=int, default=400, help="Window length; the windows do not overlap.")
    po.add_argument("-b", "--batch_size", type=int, default=1100, help="Windows per engine batch.")
    po.add_argument("--band", type=int, default=256, help="First half-width of the frame alignment's band, in CTC states; 0: the full table.")
    po.add_argument("--max-band", dest="max_band", type=int, default=8192,
                    help="Largest half-width the doubling may reach before a read is given up (0: unbounded).")
    po.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one batch of any stage, MiB.")
    po.add_argument("--dtype", default="fp32", choices=["fp32", "fp16", "fp16-w2", "fp32-split"], help="Engine arithmetic.")
    po.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    po.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                    help="Use seeded synthetic weights when the model folder has no checkpoint data.")
    po.set_defaults(func=polish)
    dm = subparsers.add_parser("demux", description="Split the called reads of a multiplexed run by barcode and cut barcode and adapter "
                               "sequence off their ends: the first and last bases of every read searched for every barcode on the GPU, "
                               "exactly, by edit distance",
                               help="Split called reads by barcode and trim their ends.")
    dm.add_argument("-i", "--input", required=True, help="Output folder of `call` (its result/ is read), or a fasta/fastq file or folder.")
    dm.add_argument("--barcodes", required=True,
                    help="FASTA of the barcodes as they read at a read's start, 1 to 64 bases each; records that share a name are spellings "
                         "of one barcode.  A file with a single adapter is plain adapter trimming into one bin.")
    dm.add_argument("-o", "--output", required=True,
                    help="Folder <barcode>.fastq per bin (.fasta when the input has no qualities), unclassified.<ext>, demux.tsv and "
                         "demux_report.json are written to.")
    dm.add_argument("--window", type=int, default=150, help="Bases of either read end that are searched (not tuned on real reads).")
    dm.add_argument("--max-err", dest="max_err", type=float, default=0.2,
                    help="An end hits when its best barcode lies within this share of the barcode's length in edits (not tuned on real reads).")
    dm.add_argument("--min-margin", dest="min_margin", type=int, default=2,
                    help="... and the best other barcode is at least this many edits worse (not tuned on real reads).")
    dm.add_argument("--require", default="either", choices=["either", "both"],
                    help="either: one end's hit names the barcode; both: the two ends must hit and agree.  Two hits that disagree are a "
                         "conflict in either mode.")
    dm.add_argument("--no-trim", dest="no_trim", action="store_true", help="Write the classified reads whole.")
    dm.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one search call, MiB.")
    dm.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    dm.set_defaults(func=demux)
    sq = subparsers.add_parser("squiggle", description="Put the reads' current levels on the genome: the samples of every called base "
                               "reduced to one level and the levels summed per position and strand on the GPU; with a control sample, "
                               "Welch's t per position (sample-compare detection of modified bases)",
                               help="Signal levels per genome position, sample comparison, k-mer level table.")
    sq.add_argument("-i", "--input", required=True, help="Output folder of `map --cigar` (its mapped.sam is read), or a SAM file.")
    sq.add_argument("-s", "--signal", required=True, help="Output folder of `call` (its raw/ is read), or a folder of .signal files.")
    sq.add_argument("-g", "--genome", required=True, help="The genome FASTA the reads were mapped to.")
    sq.add_argument("-m", "--model", type=str, default=model_default_path, help="model folder path")
    sq.add_argument("-o", "--output", required=True, help="Folder levels.tsv, squiggle_report.json and the optional outputs are written to.")
    sq.add_argument("--control", default=None, help="The control sample's `map --cigar` folder or SAM file: compare.tsv is written.")
    sq.add_argument("--control-signal", dest="control_signal", default=None, help="The control sample's `call` folder or folder of .signal files.")
    sq.add_argument("--normalize", default="mad", choices=["mad", "none"],
                    help="mad: per read, (x - median) / MAD in 1/256 units; none: the samples as they are, rounded.")
    sq.add_argument("--min-events", dest="min_events", type=int, default=5,
                    help="Fewest events both samples must have at a position and strand for it to be compared (at least 2).")
    sq.add_argument("--min-mapq", dest="min_mapq", type=int, default=0,
                    help="Drop alignments whose MAPQ is below this (`map --candidates` writes one; 255, not available, always passes).")
    sq.add_argument("--kmer", type=int, default=0, help="Also write kmer_levels.tsv, the level table of the genome K-mers (1 to 10).")
    sq.add_argument("--events", action="store_true", help="Also write events/<read>.tsv, one row per base.")
    sq.add_argument("--refine", default=None, metavar="KMER_LEVELS_TSV",
                    help="Move every base border to where the samples meet this level table (the kmer_levels.tsv of an earlier run with "
                         "--kmer): an exact banded DTW on the GPU, 64 candidates a border, of the sample and the control alike, before "
                         "anything else is computed.")
    sq.add_argument("--refine-min-events", dest="refine_min_events", type=int, default=5,
                    help="Fewest events a k-mer of the --refine table must have for its level to be used.")
    sq.add_argument("-l", "--segment_len", type=int, default=400, help="Window length; the windows do not overlap.")
    sq.add_argument("-b", "--batch_size", type=int, default=1100, help="Windows per engine batch.")
    sq.add_argument("--band", type=int, default=256, help="First half-width of the frame alignment's band, in CTC states; 0: the full table.")
    sq.add_argument("--max-band", dest="max_band", type=int, default=8192,
                    help="Largest half-width the doubling may reach before a read is given up (0: unbounded).")
    sq.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one call of any stage, MiB.")
    sq.add_argument("--dtype", default="fp32", choices=["fp32", "fp16", "fp16-w2", "fp32-split"], help="Engine arithmetic.")
    sq.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    sq.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                    help="Use seeded synthetic weights when the model folder has no checkpoint data.")
    sq.set_defaults(func=squiggle)
    lo = subparsers.add_parser("locate", description="Place raw signal on a genome without calling it: the first samples of every read "
                               "against the expected levels of both strands under a k-mer level table, by exact subsequence dynamic "
                               "time warping on the GPU",
                               help="Where on a genome raw signal comes from, by subsequence DTW against a level table.")
    lo.add_argument("-s", "--signal", required=True, help="Output folder of `call` (its raw/ is read), or a folder of .signal or .fast5 files.")
    lo.add_argument("-g", "--genome", required=True, help="The genome FASTA.")
    lo.add_argument("--table", required=True, metavar="KMER_LEVELS_TSV",
                    help="The level table: the kmer_levels.tsv of `squiggle --kmer` on a run of the same chemistry.")
    lo.add_argument("-o", "--output", required=True, help="Folder located.tsv and locate_report.json are written to.")
    lo.add_argument("--table-min-events", dest="table_min_events", type=int, default=5,
                    help="Fewest events a k-mer of the table must have for its level to be used.")
    lo.add_argument("--skip", type=int, default=0, help="Samples left out at the start of every read.")
    lo.add_argument("--prefix", type=int, default=2000,
                    help="Samples of every read that are placed (at most 16384, or 131072 under --events).  A few hundred are too few: the margins go to 0.")
    lo.add_argument("--min-samples", dest="min_samples", type=int, default=200, help="A read with fewer samples after --skip is dropped.")
    lo.add_argument("--normalize", default="mad", choices=["mad", "none"],
                    help="mad: (x - median) / MAD of the prefix in 1/256 units, as squiggle normalises a read; none: the samples as they are.")
    lo.add_argument("--max-cost", dest="max_cost", type=float, default=None,
                    help="A read whose cost per sample, in 1/256 units, is above this is unplaced (default: no limit; not tuned on real reads).")
    lo.add_argument("--min-margin", dest="min_margin", type=float, default=1.0,
                    help="A read whose second-best locus costs less than this more per sample is ambiguous (not tuned on real reads).")
    lo.add_argument("--targets", default=None, metavar="CONTIG:START-END,...",
                    help="Regions (1-based, inclusive; a bare contig is all of it): located.tsv says on_target / off_target.")
    lo.add_argument("--events", action="store_true",
                    help="Cut the prefix into events of one level each and place the events, by a DTW whose path may skip a base: "
                    "--prefix may then be up to 131072, a read keeps at most 8192 events, and costs and margins are per event.")
    lo.add_argument("--event-window", dest="event_window", type=int, default=3,
                    help="--events: samples on either side of a border that the t statistic compares, 2 to 16 (not tuned on real reads).")
    lo.add_argument("--event-threshold", dest="event_threshold", type=float, default=3.0,
                    help="--events: the least t^2 of a border (not tuned on real reads).")
    lo.add_argument("--event-radius", dest="event_radius", type=int, default=2,
                    help="--events: a border is the peak of the statistic within this many samples, 1 to 16 (not tuned on real reads).")
    lo.add_argument("--skip-penalty", dest="skip_penalty", type=int, default=150,
                    help="--events: what a base without an event costs, in 1/256 units, 0 to 65534 (not tuned on real reads).")
    lo.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one call, MiB.")
    lo.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    lo.set_defaults(func=locate)
    mc = subparsers.add_parser("modcall", description="Call modified bases per read: at every motif site of every mapped read, the samples "
                               "around the site against the window's expected levels under a canonical and under a modified k-mer level "
                               "table, by an exact dynamic time warping with free borders on the GPU; the difference of the two costs is "
                               "the call",
                               help="Per-read modified-base calls at motif sites from two k-mer level tables.")
    mc.add_argument("-i", "--input", required=True, help="Output folder of `map --cigar` (its mapped.sam is read), or a SAM file.")
    mc.add_argument("-s", "--signal", required=True, help="Output folder of `call` (its raw/ is read), or a folder of .signal files.")
    mc.add_argument("-g", "--genome", required=True, help="The genome FASTA the reads were mapped to.")
    mc.add_argument("-m", "--model", type=str, default=model_default_path, help="model folder path")
    mc.add_argument("--table", required=True, metavar="KMER_LEVELS_TSV",
                    help="The canonical level table: the kmer_levels.tsv of `squiggle --kmer` on an unmodified run.")
    mc.add_argument("--alt-table", dest="alt_table", required=True, metavar="KMER_LEVELS_TSV",
                    help="The alternative level table: the same command on a fully modified run; it must have the same k.")
    mc.add_argument("-o", "--output", required=True, help="Folder mod_calls.tsv, mod_sites.tsv and modcall_report.json are written to.")
    mc.add_argument("--motif", default="CG", help="The motif, over ACGT; on the reverse strand its occurrences in the reverse complement.")
    mc.add_argument("--motif-offset", dest="motif_offset", type=int, default=0, help="Which base of the motif is the modified one, from 0.")
    mc.add_argument("--flank", type=int, default=2,
                    help="Positions the window extends past the k-mers around a group's first and last site; a window above 16 is dropped.")
    mc.add_argument("--min-delta", dest="min_delta", type=float, default=8.0,
                    help="A (read, group) whose costs differ by at least this much per sample, in 1/256 units, is called modified or "
                         "canonical, anything else ambiguous (from a sketch on planted reads; not tuned on real reads).")
    mc.add_argument("--table-min-events", dest="table_min_events", type=int, default=5,
                    help="Fewest events a k-mer of either table must have for its level to be used.")
    mc.add_argument("--min-mapq", dest="min_mapq", type=int, default=0,
                    help="Drop alignments whose MAPQ is below this (`map --candidates` writes one; 255, not available, always passes).")
    mc.add_argument("--normalize", default="mad", choices=["mad", "none"],
                    help="mad: per read, (x - median) / MAD in 1/256 units, as squiggle normalises; none: the samples as they are, rounded.")
    mc.add_argument("-l", "--segment_len", type=int, default=400, help="Window length; the windows do not overlap.")
    mc.add_argument("-b", "--batch_size", type=int, default=1100, help="Windows per engine batch.")
    mc.add_argument("--band", type=int, default=256, help="First half-width of the frame alignment's band, in CTC states; 0: the full table.")
    mc.add_argument("--max-band", dest="max_band", type=int, default=8192,
                    help="Largest half-width the doubling may reach before a read is given up (0: unbounded).")
    mc.add_argument("--workspace-mb", dest="workspace_mb", type=int, default=4096, help="Device workspace of one call of any stage, MiB.")
    mc.add_argument("--dtype", default="fp32", choices=["fp32", "fp16", "fp16-w2", "fp32-split"], help="Engine arithmetic.")
    mc.add_argument("--device", type=int, default=0, help="HIP device ordinal.")
    mc.add_argument("--synthetic-weights", dest="synthetic_weights", action="store_true",
                    help="Use seeded synthetic weights when the model folder has no checkpoint data.")
    mc.set_defaults(func=modcall)
    return parser


def main(arguments=None):
    parser = build_parser()
    argv = list(sys.argv[1:] if arguments is None else arguments)
    args = parser.parse_args(argv)
    args.child_argv = argv                    # `--gpus N` re-runs this command line in N rank processes
    if hasattr(args, "func"):
        return args.func(args)
    parser.print_help()


if __name__ == "__main__":
    main()
