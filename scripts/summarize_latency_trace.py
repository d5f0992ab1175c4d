"""Busy time and idle gaps of a ``rocprofv3 --kernel-trace`` run of ``scripts/bench_latency.py`` (one workload, one mode).

    python scripts/summarize_latency_trace.py <trace_results.db> --samples 21 [--out summary.json]

Reads the ``kernels`` view of the rocpd database.  Kernel intervals are merged (overlapping or touching kernels count once), so
``busy_ms`` is the time the GPU had at least one kernel running; the gaps are the idle intervals between merged intervals.  A gap
longer than ``--long-gap-us`` is time where the device waited for the host (between samples: the host clock, CSR construction and
synchronisation of the benchmark; inside a sample: launches that did not keep ahead)."""
import argparse
import json
import sqlite3

import numpy as np


def summarize(db: str, samples: int, long_gap_us: float = 20.0) -> dict:
    rows = sqlite3.connect(db).execute("select start, end from kernels order by start").fetchall()
    merged = []
    for s, e in rows:
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    busy = sum(e - s for s, e in merged)
    gaps = np.array([merged[i + 1][0] - merged[i][1] for i in range(len(merged) - 1)], dtype=np.float64) / 1e3      # us
    long = gaps[gaps > long_gap_us]
    span = merged[-1][1] - merged[0][0]
    return dict(kernels=len(rows), samples=samples, busy_ms=busy / 1e6, span_ms=span / 1e6, busy_share_of_span=busy / span,
                busy_ms_per_sample=busy / 1e6 / samples, gaps=int(gaps.size),
                gap_us_median=float(np.median(gaps)) if gaps.size else None,
                gap_us_p90=float(np.percentile(gaps, 90)) if gaps.size else None,
                short_gaps_ms_total=float(gaps[gaps <= long_gap_us].sum() / 1e3),
                long_gaps=int(long.size), long_gaps_ms_total=float(long.sum() / 1e3), long_gap_threshold_us=long_gap_us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--samples", type=int, required=True)
    ap.add_argument("--long-gap-us", type=float, default=20.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = summarize(a.db, a.samples, a.long_gap_us)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
