#!/usr/bin/env python3
"""From a rocprofv3 --kernel-trace rocpd database: for each kernel named on the command line, its average duration and the average distance
from its start to the start of the launch behind it (the first launch that starts at or after its end), with that launch's name. The
difference of the two is what the boundary cost: the launch floor plus whatever the kernel left to write back.
usage: trace_gaps.py results.db <kernel name fragment>..."""
import collections
import re
import sqlite3
import sys


def short(name):
    return re.sub(r"\(.*", "", name.replace("(anonymous namespace)::", "").replace("void ", ""))


def main():
    db = sqlite3.connect(sys.argv[1])
    rows = [(short(n), s, e) for n, s, e in db.execute("select name, start, end from kernels order by start")]
    for frag in sys.argv[2:]:
        dur, dist, behind = [], [], collections.Counter()
        for i, (n, s, e) in enumerate(rows):
            if frag not in n:
                continue
            nxt = next((r for r in rows[i + 1:i + 8] if r[1] >= e), None)
            if nxt is None or nxt[1] - e > 50000:  # (the last launch of a step: what follows is the host's collect, not a boundary)
                continue
            dur.append(e - s), dist.append(nxt[1] - s), behind.update([nxt[0]])
        if dur:
            d, g = sum(dur) / len(dur) / 1e3, sum(dist) / len(dist) / 1e3
            print(f"{frag:22s} n={len(dur):4d} avg {d:8.2f} us  start-to-start {g:8.2f} us  boundary {g - d:6.2f} us  -> {behind.most_common(1)[0][0]}")


if __name__ == "__main__":
    main()
