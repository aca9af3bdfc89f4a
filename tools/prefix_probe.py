#!/usr/bin/env python3
"""bench.py with the send-free prefix switched off, or with its statistics printed.

    python tools/prefix_probe.py off   [bench.py arguments]
    python tools/prefix_probe.py stats [bench.py arguments]
    python tools/prefix_probe.py noskip [bench.py arguments]

`off` calls tw_set_prefix(0) behind every load, so the result line is the A/B
arm "this library without the prefix" measured by bench.py's own loop.  `stats`
leaves the prefix on and prints tw_prefix_stats after the last step to stderr
(T0, the snapshot's events and bytes per replica, the apply's device time and
its store rate over the batch; tw_prefix_clean_stats: the claimed slots, the
rows the last apply skipped and the bytes it stored; tw_prefix_rows_stats: the
header, run-entry and reset-valued rows it skipped beside them and the bytes
it really stored, which the stored rate is over).  `noskip` leaves the
prefix on but makes every apply store every row the sweep would have to prove
(a tw_set_prefix(1) before each run: any setter ends the last run's
verification; the reset-valued rows stay skipped).  The result line is bench.py's in both cases.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "time-warp_amd")]


def main():
    if len(sys.argv) < 2 or sys.argv[1] not in ("off", "stats", "noskip"):
        raise SystemExit(__doc__)
    mode = sys.argv.pop(1)
    import bench
    from timewarp.engine import Engine

    load, close = Engine.load, Engine.close

    def load_off(self, scn, geometry=None):
        load(self, scn, geometry)
        if geometry != "lpb":
            self.set_prefix(False)
        return self

    def close_stats(self):
        if self.ctx and self.scn is not None:
            st = self.prefix_stats()
            if st["apply_ms"] > 0:
                st["apply_TBps"] = st["bytes"] * self.scn.n_replicas / (st["apply_ms"] * 1e-3) / 1e12
                # (what the apply stored: tw_prefix_clean_stats' bytes, not the snapshot's)
                cs = self.prefix_clean_stats()
                stored = cs["bytes_stored"]
                rs = None
                if hasattr(self.lib, "tw_prefix_rows_stats"):  # (an older build under TW_LIB lacks it)
                    rs = self.prefix_rows_stats()
                    stored = rs["bytes_stored"]  # (less the header, run-entry and reset-valued rows)
                st["stored_TBps"] = stored * self.scn.n_replicas / (st["apply_ms"] * 1e-3) / 1e12
                st.update(cs)
            print(f"[prefix] {st}", file=sys.stderr, flush=True)
            if st["apply_ms"] > 0 and rs is not None:
                print(f"[prefix rows] {rs}", file=sys.stderr, flush=True)
        close(self)

    run = Engine.run

    def run_noskip(self, *a, **k):
        self.set_prefix(True)
        return run(self, *a, **k)

    if mode == "off":
        Engine.load = load_off
    elif mode == "noskip":
        Engine.run = run_noskip
    else:
        Engine.close = close_stats
    bench.main()


if __name__ == "__main__":
    main()
