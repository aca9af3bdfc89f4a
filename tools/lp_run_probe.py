"""Wall time of tw_lp_run, the library-owned window loop, on one GPU: gossip at
the size tests/test_gpu_multi.py::test_lp_run_over_shards uses (6,000 nodes,
drop_log2=4, seed=21), over four shards of device 0 (the copy transport) and
over a one-rank RCCL job.

    python tools/lp_run_probe.py                                   # this library
    TW_LIB=<parent's libtimewarp.so> python tools/lp_run_probe.py   # the parent's

Each process makes one context per transport, runs once untimed (the set-up),
then times one reset + run_lp and prints its ms, windows and ticks, checked
against the oracle's event count.  Its log: profiles/lp_run_host/ab_summary.txt."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "time-warp_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    import oracle

    from timewarp import engine, scenarios

    engine.load_library()
    scn = scenarios.gossip(6000, drop_log2=4, seed=21)
    L = int(scn.meta["lookahead_us"])
    s = engine.lp_scenario(scn)
    events = int(oracle.run(scn, trace_cap=0).result["events"])
    arms = [("copy x4", dict(devices=[0] * 4)), ("rccl x1", dict(comm=(1, 0, engine.comm_id())))]
    for name, kw in arms:
        with engine.LPEngine(s, 0, scn.n_nodes, L, **kw) as e:
            e.reset()
            e.run_lp()
            e.reset()
            t0 = time.perf_counter()
            lp = e.run_lp()
            ms = (time.perf_counter() - t0) * 1e3
            agg, _ = e.lp_results()
        assert lp.done == 1 and lp.err == 0 and int(agg["events"]) == events, (name, lp.done, lp.err)
        print(f"{os.environ.get('TW_LIB', 'lib/libtimewarp.so')}  {name}: run_lp {ms:.2f} ms, "
              f"windows {lp.windows}, ticks {lp.ticks}, events {events}", flush=True)


if __name__ == "__main__":
    main()
