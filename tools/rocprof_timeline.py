#!/usr/bin/env python3
"""Kernel timeline of the last N dispatches of a rocprofv3 run (rocpd SQLite output):
start/end relative to the first shown dispatch, queue id, duration.

usage: python tools/rocprof_timeline.py <run_results.db> [--last N] [--grep PATTERN]
           [--step-from REGEX] [--span START_REGEX END_REGEX]

--step-from REGEX: show the trace from the LAST run of consecutive dispatches whose names
match REGEX (e.g. the first window-sum kernel of the last grid step) instead of the last N.
--span START END: also print, for every traced step, the time from the start of the first
START dispatch to the start of the next END dispatch (e.g. the window-sum front end: first
window-sum kernel to the first band_coop_kernel).
"""
import argparse
import re
import sqlite3

import pandas as pd

# the first kernel of a grid step: the one-pass window sums or the two-kernel path's first
STEP_HEAD = r"wsum_onepass_kernel|wsum_upper_kernel"


def short(n: str) -> str:
    return re.sub(r"\(.*", "", re.sub(r"void |\(anonymous namespace\)::", "", n))[:60]


def spans(k: pd.DataFrame, start: str, end: str) -> list:
    """[(start_us, span_us)] per step: first START dispatch (after the previous END) to the
    start of the next END dispatch."""
    out, t0 = [], None
    for name, s in zip(k["name"], k["start"]):
        if t0 is None and re.search(start, name):
            t0 = s
        elif t0 is not None and re.search(end, name):
            out.append((t0 / 1e3, (s - t0) / 1e3))
            t0 = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--last", type=int, default=40)
    ap.add_argument("--grep", default=None)
    ap.add_argument("--step-from", default=None, metavar="REGEX")
    ap.add_argument("--span", nargs=2, default=None, metavar=("START", "END"))
    a = ap.parse_args()
    con = sqlite3.connect(a.db)
    cols = [r[1] for r in con.execute("pragma table_info(kernels)")]
    q = "queue_id" if "queue_id" in cols else ("stream_id" if "stream_id" in cols else None)
    k = pd.read_sql(f"select name, start, end{', ' + q if q else ''} from kernels order by start", con)
    if a.grep:
        k = k[k["name"].str.contains(a.grep)]
    if a.span:
        sp = spans(k, a.span[0], a.span[1])
        print(f"# span {a.span[0]} -> {a.span[1]} (start to start), us per traced step: "
              + " / ".join(f"{d:.1f}" for _, d in sp))
    if a.step_from:
        hit = [i for i, n in enumerate(k["name"]) if re.search(a.step_from, n)]
        if not hit:
            raise SystemExit(f"no dispatch matches {a.step_from!r}")
        i0 = hit[-1]
        while i0 - 1 in hit:
            i0 -= 1
        k = k.iloc[i0:].copy()
    else:
        k = k.tail(a.last).copy()
    t0 = k["start"].min()
    k["t0_us"] = (k["start"] - t0) / 1e3
    k["t1_us"] = (k["end"] - t0) / 1e3
    k["dur_us"] = (k["end"] - k["start"]) / 1e3
    k["name"] = k["name"].map(short)
    pd.set_option("display.width", 200)
    print(k[["name"] + ([q] if q else []) + ["t0_us", "t1_us", "dur_us"]].to_string(index=False))


if __name__ == "__main__":
    main()
