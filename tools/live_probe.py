"""What a live draw costs: a step of C3's shape (4,096 nodes x 65,536 replicas,
no drops) or of C2's (ping-pong, where sends are about a third of the events)
with the delays read from the link table or drawn at each send
(tw_set_live_delays).

    python tools/live_probe.py --mode table            # this library, the table
    python tools/live_probe.py --mode live             # this library, live delays
    TW_LIB=<parent's libtimewarp.so> python tools/live_probe.py --mode table
                                                       # the table as the parent runs it

Each process sets up, warms up and times K steps (reset + run to quiescence,
as bench.py times them) and prints ms per step, the step's events and sends,
and live_stats.  The two modes run different random delays, so their event
counts differ slightly; ns per send is (live - table) ms over the live run's
sends.  Its log: profiles/live_delays/probe.log."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "time-warp_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["table", "live"], default="live")
    ap.add_argument("--config", choices=["token_ring", "ping_pong"], default="token_ring")
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--replicas", type=int, default=None, help="65,536 (token_ring), 1,048,576 (ping_pong)")
    ap.add_argument("--duration-s", type=int, default=120)
    ap.add_argument("--round-trips", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed-base", type=int, default=0)
    ap.add_argument("--geometry", default=None)
    a = ap.parse_args()

    import torch

    from timewarp import scenarios
    from timewarp.engine import Engine, draw_link_table

    live = a.mode == "live"
    if a.config == "token_ring":
        R = a.replicas or 65536
        scn = scenarios.token_ring(n_nodes=a.nodes, n_replicas=R, launch_duration=a.duration_s * 1_000_000,
                                   drop_log2=0, seed_base=a.seed_base, drawer=draw_link_table, live=live)
        tie = "forkfirst"
        what = f"token ring {a.nodes} nodes x {R} replicas, {a.duration_s} s, no drops"
    else:
        R = a.replicas or (1 << 20)
        scn = scenarios.ping_pong(n_replicas=R, round_trips=a.round_trips, seed_base=a.seed_base,
                                  drawer=draw_link_table)
        tie = "fifo"
        what = f"ping-pong x {R} replicas, {a.round_trips} round trips"
    with Engine(0) as e:
        e.load(scn, geometry=a.geometry)
        if tie != "fifo" and e.geometry() not in ("wave", "lpb"):
            e.set_tie_mode(tie)
        if live:
            e.set_live_delays(scn, seed_base=a.seed_base)
        for _ in range(a.warmup):
            e.reset()
            e.run()
        ms = []
        for _ in range(a.steps):
            e.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st = e.run()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        draws = e.live_stats() if hasattr(e.lib, "tw_live_stats") else None
        lib = os.environ.get("TW_LIB") or "this tree's library"
        print(f"[live_probe] {what}; mode {a.mode}, geometry {e.geometry()}, tie {tie}, library {lib}")
        print(f"[live_probe] ms per step: mean {sum(ms) / len(ms):.2f}, min {min(ms):.2f}, max {max(ms):.2f} "
              f"over {a.steps} steps; kernel {st.kernel_ms:.2f} ms in {st.launches} launches (last step)")
        print(f"[live_probe] per step: {st.events} events, {st.sends} sends ({st.sends / max(1, st.events):.3f} "
              f"of the events), {st.replicas_error} error replicas; live_stats {draws}")


if __name__ == "__main__":
    main()
