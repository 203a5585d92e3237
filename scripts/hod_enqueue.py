#!/usr/bin/env python3
"""Host enqueue cost of a populate on the BASELINE config 2 catalogue (10^7 + 10^7, LRG, as bench.py stages it).

    python scripts/hod_enqueue.py [--calls 1000] [--reps 3] [--option NAME=VALUE ...]

Each repetition enqueues `--calls` populate_async calls back to back.  The first `--calls` / 4 fill the device queue
and are not timed; the rest are timed with the queue backed up (`enqueue_us_per_call`), then the device is waited for
(`step_us`: microseconds per populate over all `--calls`, from the first call until the device is idle).  With a backed-up queue a call
that has to wait for a free queue slot shows up in `enqueue_us_per_call` too: the number is only a host cost while it
stays below `step_us`.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--nhalo', type=int, default=10_000_000)
    ap.add_argument('--npart', type=int, default=10_000_000)
    ap.add_argument('--option', action='append', default=[], metavar='NAME=VALUE')
    args = ap.parse_args()
    from abacusutils_amd import _lib, synth
    from abacusutils_amd.hod import GRAND_HOD as G
    for o in args.option:
        k, v = o.split('=')
        _lib.set_option(k, int(v))
    tracers = {'LRG': dict(synth.LRG_PARAMS)}
    hd, pd, params = synth.synth_hod_inputs(args.nhalo, args.npart, seed=600)
    p = G.marshal_params(tracers, params, False, True)
    st = G.StagedCatalog(hd, pd)
    for _ in range(20):   # staging work, key index, steady state
        st.populate(p)
    st.wait_counts()
    runs = []
    fill = args.calls // 4
    for _ in range(args.reps):
        _lib.sync()
        ts = time.perf_counter()
        for _ in range(fill):
            st.populate_async(p)
        t0 = time.perf_counter()
        for _ in range(args.calls - fill):
            st.populate_async(p)
        t1 = time.perf_counter()
        st.wait_counts()
        _lib.sync()
        t2 = time.perf_counter()
        n = args.calls - fill
        runs.append({'enqueue_us_per_call': (t1 - t0) / n * 1e6, 'step_us': (t2 - ts) / args.calls * 1e6})
    st.free()
    print(json.dumps({'opts': args.option, 'calls': args.calls, 'runs': runs}))


if __name__ == '__main__':
    main()
