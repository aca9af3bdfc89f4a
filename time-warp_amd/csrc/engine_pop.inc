// engine_pop.inc -- the pop phase of tw_run_kernel's event loop (engine_dev.hpp),
// included as text where it runs: in the loop body itself, and, in the kernels
// with reap iterations, once more in the pop phase that follows a reap iteration.
// The including code declares `Th th; uint32_t slot = 0; bool run = false;` and
// defines TW_POP_TAIL, the vector-memory ops issued since the last record
// prefetch (the literal of this copy's counted waits).
        #ifdef TW_STATS
                tl0 = __builtin_amdgcn_s_memtime();
                pkind = 0;
        #endif
                STATL(K_ITER);  // lane-iterations, idle lanes included (pops / this = lane efficiency)
                // the rare cases (main's first run, quiescence, the event cap) behind one
                // wave-uniform branch; the common path is a single divergent region
                const bool rare = alive && (pending_main || L.live == 0 || L.d_ev >= ev_room);
                if (__builtin_amdgcn_ballot_w64(rare)) {
                    if (rare && pending_main) {  // runInSandbox main (TimedT.hs:237): runs at t=0, not a pop
                        pending_main = 0;
                        L.pf_slot = 0xFFFFFFFFu;
                        L.template fetch_rec<TW_POP_TAIL>(0, th);
                        L.rf[0] = th.r0; L.rf[WG] = th.r1; L.rf[2 * WG] = th.r2; L.rf[3 * WG] = th.r3;
                        L.hnode = th.w1;
                        run = true;
                    } else if (rare) {  // whileM_ notDone, or this launch's event cap
                        if (!LP && L.live == 0) L.status = TW_REP_DONE;  // an LP may still receive records
                        alive = false;
                    }
                }
                bool popping = alive && !rare;
                L.q1d = false;
                {
                    // PQ.minView: the min of the near root and the far sources
                    if (L.far_dirty) L.far_min();
                    const bool use_near = L.near_n != 0;
                    const int64_t tn = L.nbase + (int64_t)(L.nrk >> 32);
                    const bool use_far = L.fsrc >= 0 && (!use_near || tless(L.fmt, L.fms, tn, (uint32_t)L.nrk));
                    const int64_t t = use_far ? L.fmt : tn;
                    const uint32_t sq = use_far ? L.fms : (uint32_t)L.nrk;
                    slot = use_far ? L.fmsl : (use_near ? L.nrs : 0u);
                    STIME(ts1);
                    STADDL(K_CYC_SEL, ts1 - tl0);
                    // parked beyond t_end (an empty queue cannot happen while live > 0)
                    const bool parked = popping && ((!use_near && !use_far) || t > te);
                    alive = parked ? false : alive;
                    popping = popping && !parked;
                    // (after a reap iteration the whole wave takes the prefetch's wait
                    // here, where the popping lanes' fetch_rec would: a pop phase in
                    // which no lane pops then leaves no prefetch uncovered on any path
                    // through the compiled loops, which funnel every exit into one latch)
                    if constexpr ((TW_POP_TAIL) != TW_TAIL_VMEM)
                        asm volatile("s_waitcnt vmcnt(%0) ; tw:pf" ::"n"(TW_POP_TAIL) : "memory");
                    if (popping) {
                        {
                            const bool due = LP && use_far && L.fsrc == 0;
                            if (due) L.due_pop(th, slot, sq);
                            else L.template fetch_rec<TW_POP_TAIL>(slot, th);  // prefetched copy or HBM
                            STIME(ts2);
                            STADDL(K_CYC_FETCH, due ? 0 : ts2 - ts1);
                            STADDL(K_CYC_DUE, due ? ts2 - ts1 : 0);
                            if (due) {
                            } else if (!use_far) L.near_pop();
                            else if (L.fsrc == TW_RUNS) {
                                // (drained: the heap walk issues loads whose values go
                                // unused; left in flight, they made the compiler wait
                                // vmcnt(0) -- for the record prefetch and the last
                                // pass's stores -- at the top of every interpreter
                                // pass of every step, tools/waitcnt_audit.py)
                                L.far_pop();
                                tw_vm_drain();
                            } else L.run_pop(L.fsrc);
                            STIME(ts3);
                            STADDL(K_CYC_QPOP, ts3 - ts2);
                            if (slot == L.pf_slot) L.pf_slot = 0xFFFFFFFFu;
                            if (th.w3 != sq) {
                                STATL(K_SUPERSEDED);  // superseded by a throwTo re-stamp
                            } else {
                                STATL(K_POP);
                                // curTime .= timestamp (TimedT.hs:241-247)
                                th.w3 = 0;
                                --L.live;
                                L.now = t;
                                if (t - L.nbase > (int64_t)0x7FFFFFFF) L.near_rebase(t);
                                L.hnode = th.w1;
                                L.rf[0] = th.r0; L.rf[WG] = th.r1; L.rf[2 * WG] = th.r2; L.rf[3 * WG] = th.r3;
                                // LP phantom = the deliverer's wake, already counted and hashed by the sender
                                const bool phantom = LP && (th_flags(th) & F_PHANTOM);
                                if (!phantom) {
                                    L.final_t = LP ? (t > L.final_t ? t : L.final_t) : t;
                                    ++L.d_ev;
                                }
                                const uint32_t exc = th_exc(th);  // asyncExceptions . at tid <<.= Nothing (:252)
                                if (exc) {
                                    const int64_t val = th_xval(th);
                                    th_set_exc(th, 0);
                                    th.xl = th.xh = 0;
                                    L.q1d = true;
                                    L.hacc += term0(t, TW_KIND_EXC | exc);
                                    if (!(th_flags(th) & (F_STARTED | F_MAIN))) {  // escapes launchTimedT (:252-263)
                                        L.status = TW_REP_ABORTED;
                                        L.cs(CW_MAINEXC, exc);
                                        L.put_rec(slot, th);
                                    } else {
                                        run = L.unwind(th, slot, exc, val);
        #ifdef TW_STATS
                                        if (!run) { STATL(K_VPOP); pkind = 1; }
        #endif
                                    }
                                } else {
                                    if (!phantom) L.hacc += term0(t, TW_KIND_RESUME | th_pc(th));
                                    run = true;
                                }
                            }
                        }
                    }
                }
                if (!popping) slot = 0u;  // main's first run is slot 0; idle lanes do not use it
