"""What the consensus tests share beside the reads: the restatement's answer on every read, computed once per session, and the host
path the device vote is also compared with -- assemble.cpp behind assembly.simple_assembly_qs, np.argmax, and the vote summary
(n1, n2, q_top) by the rule of eval.qs; tests/test_consensus_cpu.py checks that eval.qs gives these very numbers to its formula."""
import functools

import numpy as np

import consensus_cases
import consensus_ref


@functools.lru_cache(maxsize=None)
def reference():
    """(name, kernal) -> consensus_ref.consensus of the read"""
    return {(name, kernal): consensus_ref.consensus(segs, qs, kernal) for name, segs, qs, kernal in consensus_cases.cases()}


def vote_summary(cons, cqs):
    """eval.qs's rule: the LAST of the largest counts is the winner, n2 the largest count beside it, q_top the winner's quality sum"""
    cols = np.arange(cons.shape[1])
    top = cons.shape[0] - 1 - np.argmax(cons[::-1], axis=0)
    rest = cons.copy()
    rest[top, cols] = -1.0
    return cons[top, cols], rest.max(axis=0), cqs[top, cols]


def host_consensus(segments, qs, kernal):
    """-> (base, n1, n2, q_top, counts, qsum) of the host path"""
    from chiron_amd import assembly
    cons, cqs = assembly.simple_assembly_qs(segments, qs.reshape(-1, 1), 0.975, kernal=kernal)
    n1, n2, q_top = vote_summary(cons, cqs)
    return np.argmax(cons, axis=0), n1, n2, q_top, cons, cqs
