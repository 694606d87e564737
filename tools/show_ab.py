#!/usr/bin/env python3
"""Summarise an interleaved A/B file of bench.py lines ({"side", "run", "line"} per row): per
side the values, their median and spread.  python tools/show_ab.py FILE.jsonl"""
import json
import sys

rows = [json.loads(l) for l in open(sys.argv[1]) if l.strip()]
for side in sorted({r["side"] for r in rows}):
    v = sorted(r["line"]["value"] for r in rows if r["side"] == side)
    print(f"{sys.argv[1]} {side}: median {v[len(v) // 2]:.1f} min {v[0]:.1f} max {v[-1]:.1f} "
          f"{rows[0]['line']['unit']}  values {[round(x, 1) for x in v]}")
