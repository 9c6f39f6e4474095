// ldpc5g_dec_frame_iter.h — the decode iterations of frame_body (ldpc5g_dec_frame.h), included
// inside it by workgroup-uniform choices: with DEAD = true (the dead-extension-row shortcuts, for
// a codeblock with a dead row) and DEAD = false, both with FIRST = false; and once with
// FIRST = true, DEAD = false: iteration 0 alone, peeled in front of the loop when the punctured
// columns 0 and 1 are +0.0 (pc == 2).  A textual include rather than a generic lambda: the lambda
// form spills VGPRs in the plain kernel (measured ~1 % slower).
// No include guard on purpose; not a standalone header.
//
// FIRST relies on the state being zero and on LQ(0) = LQ(1) = +0.0:
//  - r_old = +0.0 on every edge, so q = LQ - (+0.0) = LQ bit for bit (-0.0 included): no state
//    read, select, sign application, sign-word walk or subtraction.
//  - A row with a punctured column (every BG1 row, all BG2 rows but five) has min1 = |+0.0| at its
//    first punctured edge, which is edge 0 (edges are in column order, `aq < min1` is strict), and
//    min2 = min |LQ| over its other edges (0 when it holds both punctured columns).  Per core edge
//    that leaves the parity compare, the sign collect and one v_min_f64.
//  - Such a row sends +-mA = +-alpha * clamp(0) to every column >= 2 and, when it holds both
//    punctured columns, +-0 to those too.  frame_body takes this path only when alpha * clamp(0)
//    is +-0, so all those messages are +-0 and phase B drops them: a sum that starts at +0.0 never
//    becomes -0.0 (x + (-x) rounds to +0.0), so S + (+-0) = S for every partial sum.  Columns no
//    other row touches become LLR + (+0.0); only a row's message to its single punctured column
//    (+-mB) enters the register sum S.  With no LDS add there is no group barrier.
//  - The syndrome flag is its own word (never reset): without phase-B barriers a reset of flagA
//    could overtake another wave's read of it.
//
// FUSED (FIRST with BG1, where every row holds a punctured column; frame_body takes it for L >= 2):
// iteration 0 together with iteration 1's phase A.  After iteration 0 every message into a column
// >= 2 is +-0, so the LQ image of those columns is LLR + (+0.0) (the prologue stored that) and in
// iteration 1 every edge but a row's first punctured one has r_old = +-0: |q| and q < 0 on the
// non-punctured edges are what iteration 0 walked.
//  - The pass (rowA_fused): each owned row in the zero-state form over its non-punctured edges;
//    (min1', min2'), their sign word and argmin' are parked in the row's state slots.  Iteration
//    0's own state is implicit: mA = alpha * clamp(0) = +-0, mB = alpha * clamp(min1'), idx = 0.
//  - After the syndrome barrier: S = the row-ordered sum of +-mB over the rows with exactly one
//    punctured column H (first_msg), T(0) + S into the image of column H, one barrier.
//  - The combine (rowC): iteration 1's state of each owned row from the parked minima and its
//    punctured edge(s), q_0 = (T(0) + S) - (+-mB), or the LQ entries themselves for a row with
//    both (LQ - (+-0) = LQ, no image entry is -0.0).  The punctured edges come first in edge
//    order and `aq < min1` is strict, so they keep the argmin on a tie.
//  - The loop (FIRST = false) is then entered at it = 1 with skipA set: its first trip skips
//    phase A and goes on at the barrier before the syndrome test.

    auto rdead = [&](int i) -> bool { return DEAD && i >= 4 && ((live_x >> (i - 4)) & 1u) == 0; };
    int* const flagI = FIRST ? flagA + 2 : flagA;
    constexpr bool FUSED = FIRST && BG == 1;   // the fused start, see the top
    // ext LLR ring: slot p % XP holds the LLR of the half's ext row p, loaded XP rows ahead
    // (FIRST: its own, deeper ring — those loads come from HBM, the loop's from L2)
    constexpr int XP = FIRST ? kFrXPreFirst : kXPre > 0 ? kXPre : 1;
    // The ring and the wrap-table offsets of the stream live across the loop's back edge: with PRE a
    // trip issues the next trip's cold-start loads (the ring's first XP rows, the stream's first
    // kFrDT table reads) before its last group barrier, and the next trip's phase A finds them
    // there (`pre`: every trip but the loop's first).  Neither depends on anything the loop
    // writes: the LLRs are the kernel's input and the wrap table is constant until the final pass.
    // A workgroup that leaves the loop has loaded XP + kFrDT values for nothing.
    constexpr bool PRE = kSeamPre && !FIRST && !KDEAD;
    // the other steps of LDPC5G_FR_SEAM (ldpc5g_dec_frame.h), in the plain kernels only: the
    // rate-matched (KDEAD) kernels run without them (their one --full line measured with steps
    // 1, 4, 8 was slower, 2.087 against 2.011 ms per batch)
    constexpr bool SBAR = kSeamBar && !KDEAD, SLF = kSeamLf && !KDEAD, SUPD = kSeamUpd && !KDEAD,
                   SPRIO = kSeamPrio && !KDEAD;
    T xr[XP];
    uint32_t tbs[kFrDT];
    bool pre = false;
    for (; it < (FIRST ? (L < 1 ? L : 1) : L); ++it) {
        // opaque per iteration: otherwise LICM hoists hundreds of loop-invariant addresses
        uint32_t sb = sb0, sbw = sbw0, tz = tz0;
        int sv = s;
        asm volatile("" : "+v"(sb));
        asm volatile("" : "+v"(sbw));
        asm volatile("" : "+v"(tz));
        asm volatile("" : "+v"(sv));
        auto rot = [&](int c) -> uint32_t { return fr_rot(sb, sbw, c); };
        // check node of row i run by this thread: (s - off[i]) mod Zc
        auto xpos = [&](int i) -> int {
            const int c = (Z - kFrPlan<BG>.off[i]) % Z;
            if (c == 0) return sv;
            return (int)min((uint32_t)(sv + c), (uint32_t)(sv + c - Z));
        };
        auto llrx = [&](int i) -> T { return ldg(lrow_x, i * Z + xpos(i)); };
        bool fail = false;
        uint64_t hdx = 0;   // hard decisions of the owned extension columns (LQ_old)
        const bool runA = FIRST || !skipA;   // after the fused start: iteration 1's state is there,
        if (!runA) hdx = hdx_keep;           // and its decisions are those of the start's pass

        auto xload = [&](auto hc, auto pc_) {
            constexpr int hh = decltype(hc)::value, p = decltype(pc_)::value;
            if constexpr (p < kFrPlan<BG>.nx[hh]) xr[p % XP] = llrx(kFrPlan<BG>.xlist[hh][p]);
        };
        // ---- phase A: new row state from LQ_old (:117-123, _min_sum_process :186-202).  The
        // half's core-edge stream (FrStream): entry p's wrap-table offset is read kFrDT positions
        // ahead and its LQ kFrDA ahead, across row boundaries (slots p % kFrDT, p % kFrDA)
        // sg: the row's sign bits, old and new in one shift register.  It starts as the old
        // signs left-aligned (get_state: edge 0 in bit 31) and moves left once per edge: that
        // drops edge k's old sign (used for rold_k), brings edge k + 1's to bit 31 and takes
        // edge k's new sign in at bit 0.  After the row's d edges its low d bits are the new
        // signs, edge 0 in bit d - 1.
        struct RowSt {
            T mA, mB, min1, min2;
            uint32_t sg, idxo, idx;
            bool par;
        };
        T abq[kFrDA];
        auto sload_t = [&](auto hc, auto pc_) {
            constexpr int hh = decltype(hc)::value, p = decltype(pc_)::value;
            if constexpr (p < kFrStr<BG>.n[hh]) {
                constexpr int i = kFrStr<BG>.row[hh][p], k = kFrStr<BG>.k[hh][p];
                if constexpr (!(FIRST && P::COL[P::RS[i] + k] < 2))   // FIRST: LQ(0), LQ(1) known
                    tbs[p % kFrDT] = *(lds_u32*)(uintptr_t)(tz + (uint32_t)fr_cof<BG>(i, k) * 4u);
            }
        };
        auto sload_a = [&](auto hc, auto pc_) {
            constexpr int hh = decltype(hc)::value, p = decltype(pc_)::value;
            if constexpr (p < kFrStr<BG>.n[hh]) {
                constexpr int i = kFrStr<BG>.row[hh][p], k = kFrStr<BG>.k[hh][p];
                if constexpr (!(FIRST && P::COL[P::RS[i] + k] < 2))
                    abq[p % kFrDA] = at((uint32_t)(P::COL[P::RS[i] + k] * kFrColB) + tbs[p % kFrDT]);
            }
        };
        // core edge k of row i: the stream moved on by one; its LQ entry first
        auto sskip = [&](auto ic, auto kc) {
            constexpr int i = decltype(ic)::value, k = decltype(kc)::value;
            constexpr int hh = kFrPlan<BG>.owner[i], p = kFrStr<BG>.start[i] + k;
            sload_a(std::integral_constant<int, hh>{}, std::integral_constant<int, p + kFrDA>{});
            sload_t(std::integral_constant<int, hh>{}, std::integral_constant<int, p + kFrDT>{});
        };
        auto snext = [&](auto ic, auto kc) -> T {
            constexpr int i = decltype(ic)::value, k = decltype(kc)::value;
            const T a = abq[(kFrStr<BG>.start[i] + k) % kFrDA];
            sskip(ic, kc);
            return a;
        };
        auto rowA = [&](auto ic) {
            constexpr int i = decltype(ic)::value, e0 = P::RS[i], d = kFrPlan<BG>.deg(i);
            static_assert(d <= 19, "old and new signs of a row share one 32-bit register");
            RowSt r;
            get_state(ic, r.mA, r.mB, r.sg, r.idxo);
            r.min1 = FT<T>::inf(), r.min2 = FT<T>::inf();
            r.idx = 0, r.par = false;
            sfor<0, d>([&](auto kc) {
                constexpr int k = decltype(kc)::value, j = P::COL[e0 + k];
                const T rold = xsign_v(pick(r.idxo == (uint32_t)k, r.mB, r.mA), r.sg, mv);
                T a;
                if constexpr (j < KC) {
                    a = snext(ic, kc);
                    __builtin_amdgcn_sched_barrier(0);
                    r.par ^= a < T(0);
                } else {
                    constexpr int hh = kFrPlan<BG>.owner[i], p = kFrPlan<BG>.xpos[i];
                    a = xr[p % XP] + rold;   // LQ of a degree-1 column = LLR + its only r
                    xload(std::integral_constant<int, hh>{}, std::integral_constant<int, p + XP>{});
                    hdx |= (uint64_t)(a < T(0)) << (i - 4);
                    r.par ^= a < T(0);
                }
                const T q = a - rold;
                const T aq = fabs(q);
                r.idx = aq < r.min1 ? (uint32_t)k : r.idx;
                asm volatile("" : "+v"(r.idx));
                r.sg = __builtin_amdgcn_alignbit(r.sg, FT<T>::sbits(q), 31);
                two_min(r.min1, r.min2, aq);
            });
            fail |= r.par;
            T x1 = r.min1, x2 = r.min2;
            if constexpr (OFS) {
                x1 = r.min1 - beta, x2 = r.min2 - beta;   // max(minv - beta, 0) (:201)
                x1 = x1 > T(0) ? x1 : T(0), x2 = x2 > T(0) ? x2 : T(0);
            }
            // above the d new signs sg holds zeros (get_state's word is p << (32 - d): nothing
            // below the old signs), except in the high field of a shared word (ph == 2,
            // p << (16 - d)): there the other row's field lay below and sits in bits 16.. now
            constexpr uint32_t dm = (1u << d) - 1u;
            uint32_t negs = r.sg;
            if constexpr (!kFrPlan<BG>.lds[i] && kFrPlan<BG>.ph[i] == 2) negs &= dm;
            const uint32_t sgn = 0u - (__builtin_popcount(negs) & 1u);   // the row's sign product
            put_state(ic, alpha * x1, alpha * x2, (r.sg ^ sgn) & dm, r.idx);
        };
        // a dead extension row: LQ_ext = 0 + r_old_ext (its syndrome bit), q_core = LQ - (+-0); the
        // new state as the full update leaves it up to zero signs (ldpc5g_dec_flood.h rowA_dead)
        auto rowA_dead = [&](auto ic) {
            constexpr int i = decltype(ic)::value, e0 = P::RS[i], d = kFrPlan<BG>.deg(i);
            T mA, mB;
            uint32_t u, idxo;
            get_state(ic, mA, mB, u, idxo);
            const T rext = xsign_v(pick(idxo == (uint32_t)(d - 1), mB, mA), u << (d - 1), mv);
            constexpr int hh = kFrPlan<BG>.owner[i], p = kFrPlan<BG>.xpos[i];
            xload(std::integral_constant<int, hh>{}, std::integral_constant<int, p + XP>{});   // keep the ring moving
            const T ax = T(0) + rext;
            hdx |= (uint64_t)(ax < T(0)) << (i - 4);
            bool par = ax < T(0);
            T mn = FT<T>::inf();
            uint32_t sx = 0;
            sfor<0, d>([&](auto kc) {
                constexpr int k = decltype(kc)::value, j = P::COL[e0 + k];
                if constexpr (j < KC) {
                    const T a = snext(ic, kc);
                    par ^= a < T(0);
                    mn = fmin(mn, fabs(a));
                    sx ^= FT<T>::sbits(a);
                }
            });
            fail |= par;
            T x2 = mn;
            if constexpr (OFS) {
                x2 = mn - beta;
                x2 = x2 > T(0) ? x2 : T(0);
            }
            put_state(ic, T(0), alpha * x2, sx >> 31, (uint32_t)(d - 1));
        };
        // FIRST: the two row forms of the zero state (see the top).  LQ of edge k: a core entry
        // from the stream, or LLR + r_old = LLR + (+0.0) of the extension column (-0.0 -> +0.0)
        auto edge0 = [&](auto ic, auto kc) -> T {
            constexpr int i = decltype(ic)::value, k = decltype(kc)::value;
            if constexpr (P::COL[P::RS[i] + k] < KC) {
                return snext(ic, kc);
            } else {
                constexpr int hh = kFrPlan<BG>.owner[i], p = kFrPlan<BG>.xpos[i];
                const T a = xr[p % XP] + T(0);
                xload(std::integral_constant<int, hh>{}, std::integral_constant<int, p + XP>{});
                hdx |= (uint64_t)(a < T(0)) << (i - 4);
                return a;
            }
        };
        // the row's new state from its minima x1 <= x2: alpha * max(x - beta, 0) (:201), the signs
        auto put_first = [&](auto ic, bool par, T x1, T x2, uint32_t negs, uint32_t idx) {
            constexpr int d = kFrPlan<BG>.deg(decltype(ic)::value);
            fail |= par;
            if constexpr (OFS) {
                x1 = x1 - beta, x2 = x2 - beta;
                x1 = x1 > T(0) ? x1 : T(0), x2 = x2 > T(0) ? x2 : T(0);
            }
            const uint32_t sgn = 0u - (__builtin_popcount(negs) & 1u);
            put_state(ic, alpha * x1, alpha * x2, negs ^ (sgn & ((1u << d) - 1u)), idx);
        };
        auto rowA_punct = [&](auto ic) {   // a row with a punctured column: min1 = 0 at edge 0
            constexpr int i = decltype(ic)::value, e0 = P::RS[i], d = kFrPlan<BG>.deg(i);
            constexpr int npun = (kFrPlan<BG>.kc[0][i] >= 0) + (kFrPlan<BG>.kc[1][i] >= 0);
            T mn = npun > 1 ? T(0) : FT<T>::inf();   // min2: the second punctured edge is |+0.0|
            uint32_t negs = 0;   // the punctured edges come first and shift in zeros
            bool par = false;
            sfor<0, d>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                if constexpr (P::COL[e0 + k] < 2) {
                    static_assert(k < npun, "punctured edges first");
                    sskip(ic, kc);
                } else {
                    const T a = edge0(ic, kc);
                    par ^= a < T(0);
                    negs = __builtin_amdgcn_alignbit(negs, FT<T>::sbits(a), 31);
                    if constexpr (npun == 1) mn = fmin(mn, fabs(a));
                }
            });
            put_first(ic, par, T(0), mn, negs, 0u);
        };
        auto rowA_zero = [&](auto ic) {   // any row on the zero state: rowA with r_old = +0.0
            constexpr int i = decltype(ic)::value, d = kFrPlan<BG>.deg(i);
            T min1 = FT<T>::inf(), min2 = FT<T>::inf();
            uint32_t idx = 0, negs = 0;
            bool par = false;
            sfor<0, d>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                const T a = edge0(ic, kc);
                par ^= a < T(0);
                const T aq = fabs(a);
                idx = aq < min1 ? (uint32_t)k : idx;
                negs = __builtin_amdgcn_alignbit(negs, FT<T>::sbits(a), 31);
                two_min(min1, min2, aq);
            });
            put_first(ic, par, min1, min2, negs, idx);
        };
        // FUSED, the pass: the zero-state row over its non-punctured edges.  It parks the raw
        // (min1', min2'), their sign word and argmin' in the row's state slots.
        auto rowA_fused = [&](auto ic) {
            constexpr int i = decltype(ic)::value, e0 = P::RS[i], d = kFrPlan<BG>.deg(i);
            constexpr int npun = (kFrPlan<BG>.kc[0][i] >= 0) + (kFrPlan<BG>.kc[1][i] >= 0);
            static_assert(!FUSED || npun >= 1, "every row of the fused start holds a punctured column");
            T min1 = FT<T>::inf(), min2 = FT<T>::inf();
            uint32_t idx = 0, negs = 0;   // the punctured edges come first and shift in zeros
            bool par = false;
            sfor<0, d>([&](auto kc) {
                constexpr int k = decltype(kc)::value;
                if constexpr (P::COL[e0 + k] < 2) {
                    static_assert(k < npun, "punctured edges first");
                    sskip(ic, kc);
                } else {
                    const T a = edge0(ic, kc);
                    par ^= a < T(0);
                    const T aq = fabs(a);
                    idx = aq < min1 ? (uint32_t)k : idx;
                    asm volatile("" : "+v"(idx));
                    negs = __builtin_amdgcn_alignbit(negs, FT<T>::sbits(a), 31);
                    two_min(min1, min2, aq);
                }
            });
            fail |= par;
            put_state(ic, min1, min2, negs, idx);
        };
        // FUSED: iteration 0's message to the row's single punctured column, +-mB, from the parked
        // min1' and sign word (edge 0's own sign bit is 0, so its sign is the row's sign product);
        // alpha * max(x - beta, 0) as in put_first
        auto first_msg = [&](T x, uint32_t negs) -> T {
            if constexpr (OFS) {
                x = x - beta;
                x = x > T(0) ? x : T(0);
            }
            return xsign_v(alpha * x, (uint32_t)__builtin_popcount(negs) << 31, mv);
        };
        // FUSED, the combine: iteration 1's state of the row from the parked minima and the
        // punctured edge(s).  lqo: this thread's entry of its half's punctured column, T(0) + S.
        // An image entry is LLR + (+0.0) or T(0) + S, never -0.0, so its sign bit is its `< 0`,
        // the parked word's parity is the parity of the non-punctured edges, and
        // LQ - (+-0) = LQ bit for bit on the edges of a row with both punctured columns.
        auto rowC = [&](auto ic, T lqo) {
            constexpr int i = decltype(ic)::value, e0 = P::RS[i], d = kFrPlan<BG>.deg(i);
            constexpr int npun = (kFrPlan<BG>.kc[0][i] >= 0) + (kFrPlan<BG>.kc[1][i] >= 0);
            T m1, m2;
            uint32_t u, idx;
            get_state(ic, m1, m2, u, idx);
            uint32_t negs = u >> (32 - d);
            bool par = __builtin_popcount(negs) & 1u;
            auto lqp = [&](auto kc) -> T {   // LQ of the punctured edge k
                constexpr int k = decltype(kc)::value, j = P::COL[e0 + k], c = fr_cof<BG>(i, k);
                static_assert(j < 2 && k < npun, "punctured edges first");
                if constexpr (j == kFrPlan<BG>.owner[i] && c == 0) return lqo;
                else return at((uint32_t)(j * kFrColB) + rot(c));
            };
            if constexpr (npun == 1) {
                const T a0 = lqp(std::integral_constant<int, 0>{});
                const T q0 = a0 - first_msg(m1, negs);
                const T aq0 = fabs(q0);
                par ^= a0 < T(0);
                idx = m1 < aq0 ? idx : 0u;   // edge 0 comes first: it keeps the argmin on a tie
                two_min(m1, m2, aq0);
                negs |= (FT<T>::sbits(q0) >> 31) << (d - 1);
            } else {
                const T a0 = lqp(std::integral_constant<int, 0>{}), a1 = lqp(std::integral_constant<int, 1>{});
                const T aq0 = fabs(a0), aq1 = fabs(a1);
                par ^= a0 < T(0);
                par ^= a1 < T(0);
                idx = m1 < aq1 ? idx : 1u;
                idx = fmin(m1, aq1) < aq0 ? idx : 0u;
                two_min(m1, m2, aq0);
                two_min(m1, m2, aq1);
                negs |= ((FT<T>::sbits(a0) >> 31) << (d - 1)) | ((FT<T>::sbits(a1) >> 31) << (d - 2));
            }
            put_first(ic, par, m1, m2, negs, idx);
        };
        // phase A's cold start: the loads that need no LDS data of this trip
        auto cold_start = [&](auto hc) {
            sfor<0, XP>([&](auto pc_) { xload(hc, pc_); });
            sfor<0, kFrDT>([&](auto pc_) { sload_t(hc, pc_); });
        };
        if (active && runA) {
            per_half([&](auto hc) {
                if (!(PRE && pre)) cold_start(hc);   // else: issued by the trip before
                sfor<0, kFrDA>([&](auto pc_) { sload_a(hc, pc_); });   // LQ: behind the barrier
            });
            sfor<0, MB>([&](auto ic) {   // one branch per row: bounded live ranges
                constexpr int i = decltype(ic)::value;
                if (h == kFrPlan<BG>.owner[i]) {
                    if constexpr (SPRIO) {
                        // a wave that is behind the others of its SIMD issues first (ldpc5g_dec_frame.h)
                        constexpr int pr = fr_prio<BG>(i);
                        __builtin_amdgcn_s_setprio(pr);
                    }
                    if constexpr (FUSED) {
                        rowA_fused(ic);
                    } else if constexpr (FIRST) {
                        if constexpr (fr_punct<BG>(i)) rowA_punct(ic);
                        else rowA_zero(ic);
                    } else if constexpr (DEAD && i >= 4) {
                        if (rdead(i)) rowA_dead(ic);
                        else rowA(ic);
                    } else {
                        rowA(ic);
                    }
                }
            });
            if constexpr (SPRIO) __builtin_amdgcn_s_setprio(0);
            if (fail) *flagI = 1;
        }
        // the core LLRs of the LQ update.  SLF: issued before the barrier, so that they are
        // on their way while the workgroup waits for it and for the flag's round trip (a
        // codeblock that the syndrome test then decides has loaded them for nothing); else after
        // the test.  Either way phase B hides the rest of their latency.
        T lf[KH];
        auto load_lf = [&]() {
#pragma unroll
            for (int jj = 0; jj < KH; ++jj) {
                const int j = jcol(jj);
                lf[jj] = ldg(lrow, (j < pc ? 0 : j - pc) * Z + sv);
            }
        };
        if constexpr (SLF && !FUSED) {   // FUSED: the image of columns >= 2 holds LLR + (+0.0) already
            if (active) load_lf();
        }
        lds_barrier();
        // ---- the syndrome of LQ_old decides (:107-114): output its hard decisions
        if (active && *flagI == 0) {
            hdx_keep = hdx;   // the LQ image stays frozen (no phase B) for the decisions
            if (t == 0) status[out] = 1, iters[out] = it;
            active = false;
        }

        // ---- phase B: Lr.sum(axis=0) in row order (:126).  Columns >= 2: ds_add into the LQ
        // image, one barrier per group; column h: this thread's register sum S.
        auto msg = [&](T a, T b, uint32_t u, uint32_t idx, auto kc) -> T {   // r of edge k
            constexpr int k = decltype(kc)::value;
            return xsign_v(pick(idx == (uint32_t)k, b, a), u << k, mv);
        };
        auto add_to = [&](auto ic, auto kc, T r, uint32_t ent) {   // column of edge k of row i
            constexpr int i = decltype(ic)::value, k = decltype(kc)::value, j = P::COL[P::RS[i] + k];
            lds_T& acc = at((uint32_t)(j * kFrColB) + ent);
            // FIRST: only the rows without a punctured column add
            if constexpr ((FIRST ? fr_first_free<BG>(j) : kFrPlan<BG>.first_row[j]) == i) acc = T(0) + r;
            else __hip_atomic_fetch_add(&acc, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        };
        T S = T(0);
        if constexpr (!SLF && !FUSED) {
            if (active) load_lf();
        }
        if constexpr (FUSED) {
            // iteration 0's column sums: rows in order, a row with one punctured column H gives S
            // its message (from the parked min1'); every other message is +-0 and is dropped
            T lqo = T(0);
            if (active) {
                hdx_keep = hdx;   // iteration 1 decides on the same LLR + (+0.0) entries
                per_half([&](auto hc) {
                    constexpr int H = decltype(hc)::value;
                    sfor<0, MB>([&](auto ic) {
                        constexpr int i = decltype(ic)::value, d = kFrPlan<BG>.deg(i);
                        if constexpr (kFrPlan<BG>.kc[H][i] >= 0 && !kFrPlan<BG>.both(i)) {
                            static_assert(kFrPlan<BG>.kc[H][i] == 0, "the punctured edge first");
                            T a, b;
                            uint32_t u, idx;
                            if constexpr (kFrPlan<BG>.lds[i]) {
                                lds_get(ic, rot((Z - fr_pf<BG>(i, H)) % Z), a, b, u, idx);
                            } else {
                                static_assert(kFrPlan<BG>.owner[i] == H && kFrPlan<BG>.fr[i] == H, "own frame");
                                get_state(ic, a, b, u, idx);
                            }
                            S = S + first_msg(a, u >> (32 - d));
                        }
                    });
                });
                lqo = T(0) + S;   // punctured columns: LLR 0 (:43)
                at((uint32_t)(h * kFrColB) + sb) = lqo;
            }
            lds_barrier();
            // ---- iteration 1's phase A: each owned row's parked minima and its punctured edge(s)
            fail = false;
            if (active) {
                sfor<0, MB>([&](auto ic) {
                    if (h == kFrPlan<BG>.owner[decltype(ic)::value]) rowC(ic, lqo);
                });
                if (fail) *flagA = 1;   // read after the loop's first barrier
            }
        }
        if constexpr (FIRST && !FUSED) {
            // rows in order: a row with one punctured column H gives S its message (+-mB); a row
            // with both sends only +-0; a row with none adds as in the general code, then a barrier
            // (its columns may meet the next such row's)
            sfor<0, MB>([&](auto ic) {
                constexpr int i = decltype(ic)::value, e0 = P::RS[i], d = kFrPlan<BG>.deg(i);
                if constexpr (!fr_punct<BG>(i)) {
                    static_assert(!kFrPlan<BG>.lds[i], "a row without a punctured column is a VGPR row");
                    if (active && h == kFrPlan<BG>.owner[i]) {
                        T a, b;
                        uint32_t u, idx;
                        get_state(ic, a, b, u, idx);
                        sfor<0, d>([&](auto kc) {
                            constexpr int k = decltype(kc)::value, j = P::COL[e0 + k];
                            if constexpr (j < KC) add_to(ic, kc, msg(a, b, u, idx, kc), rot(fr_cof<BG>(i, k)));
                        });
                    }
                    lds_barrier();
                } else if constexpr (!kFrPlan<BG>.both(i)) {
                    if (active) {
                        per_half([&](auto hc) {
                            constexpr int H = decltype(hc)::value;
                            if constexpr (kFrPlan<BG>.kc[H][i] >= 0) {
                                T a, b;
                                uint32_t u, idx;
                                if constexpr (kFrPlan<BG>.lds[i]) {
                                    lds_get(ic, rot((Z - fr_pf<BG>(i, H)) % Z), a, b, u, idx);
                                } else {
                                    static_assert(kFrPlan<BG>.owner[i] == H && kFrPlan<BG>.fr[i] == H, "own frame");
                                    get_state(ic, a, b, u, idx);
                                }
                                S = S + msg(a, b, u, idx, std::integral_constant<int, kFrPlan<BG>.kc[H][i]>{});
                            }
                        });
                    }
                }
            });
            // ---- LQ = LLRin + sum (:126): a column no row added into holds LLR + (+0.0)
            if (active) {
                per_half([&](auto hc) {
                    constexpr int H = decltype(hc)::value;
                    sfor<0, KH>([&](auto jc) {
                        constexpr int jj = decltype(jc)::value, j = jj == 0 ? H : jj + 1 + H * (KH - 1);
                        lds_T& x = at((uint32_t)(j * kFrColB) + sb);
                        if constexpr (jj == 0) x = T(0) + S;   // punctured columns: LLR 0 (:43)
                        else if constexpr (fr_first_free<BG>(j) >= 0) x = lf[jj] + x;
                        else x = lf[jj] + T(0);
                    });
                });
            }
        }
        if (!FIRST && active) {
            // hand-offs: the other column's message of this half's rows with both columns
            per_half([&](auto hc) {
                constexpr int H = decltype(hc)::value;
                sfor<0, MB>([&](auto ic) {
                    constexpr int i = decltype(ic)::value;
                    if constexpr (kFrPlan<BG>.ho[i] >= 0 && kFrPlan<BG>.owner[i] == H) {
                        if (rdead(i)) return;   // its messages are +-0: nothing to hand over
                        constexpr int k = kFrPlan<BG>.kc[1 - H][i];
                        T a, b;
                        uint32_t u, idx;
                        get_state(ic, a, b, u, idx);
                        at((uint32_t)kFrPlan<BG>.hb(kFrPlan<BG>.ho[i]) + rot(fr_cof<BG>(i, k))) =
                            msg(a, b, u, idx, std::integral_constant<int, k>{});
                    }
                });
            });
        }
        sfor<0, FIRST ? 0 : kFrPlan<BG>.ng>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            constexpr uint64_t gx = fr_group_xmask<BG>(g);
            const bool gdead = DEAD && gx != 0 && (live_x & gx) == 0;   // adds nothing: no barrier
            if (active && !gdead) {
                per_half([&](auto hc) {
                    constexpr int H = decltype(hc)::value;
                    sfor<kFrPlan<BG>.gstart[g], kFrPlan<BG>.gstart[g + 1]>([&](auto ic) {
                        constexpr int i = decltype(ic)::value, e0 = P::RS[i], d = kFrPlan<BG>.deg(i);
                        if (rdead(i)) return;   // +-0 messages: no add changes a sum
                        if constexpr (kFrPlan<BG>.lds[i]) {
                            // both halves: column H's message and this half's share of the edges of
                            // columns >= 2, from the state at check node (s - Pf) mod Zc, Pf = V(i, H)
                            constexpr int Pf = fr_pf<BG>(i, H);
                            T a, b;
                            uint32_t u, idx;
                            lds_get(ic, rot((Z - Pf) % Z), a, b, u, idx);
                            sfor<0, d>([&](auto kc) {
                                constexpr int k = decltype(kc)::value, j = P::COL[e0 + k];
                                if constexpr (j == H) {
                                    S = S + xsign_v(pick(idx == (uint32_t)k, b, a), u, mv);
                                } else if constexpr (fr_item<BG>(H, i, k)) {
                                    add_to(ic, kc, xsign_v(pick(idx == (uint32_t)k, b, a), u, mv),
                                           rot((fr_sft<BG>(i, k) - Pf + Z) % Z));
                                }
                                asm("v_add_u32 %0, %1, %1" : "=v"(u) : "v"(u));   // u <<= 1
                            });
                        } else if constexpr (kFrPlan<BG>.owner[i] == H) {
                            // this half's VGPR row in frame H: column H's entry is this thread's own
                            T a, b;
                            uint32_t u, idx;
                            get_state(ic, a, b, u, idx);
                            sfor<0, d>([&](auto kc) {
                                constexpr int k = decltype(kc)::value, j = P::COL[e0 + k];
                                if constexpr (j == H) {
                                    S = S + xsign_v(pick(idx == (uint32_t)k, b, a), u, mv);
                                } else if constexpr (j >= 2 && j < KC) {
                                    add_to(ic, kc, xsign_v(pick(idx == (uint32_t)k, b, a), u, mv), rot(fr_cof<BG>(i, k)));
                                }
                                asm("v_add_u32 %0, %1, %1" : "=v"(u) : "v"(u));
                            });
                        } else if constexpr (kFrPlan<BG>.ho[i] >= 0 && kFrPlan<BG>.kc[H][i] >= 0) {
                            S = S + at((uint32_t)kFrPlan<BG>.hb(kFrPlan<BG>.ho[i]) + sb);   // the owner's hand-off
                        }
                    });
                });
            }
            if constexpr (PRE && g == kFrPlan<BG>.ng - 1) {
                // the next trip's cold start, on its way through the last group barrier, the LQ
                // update and the loop's closing barrier
                if (active && it + 1 < L) per_half(cold_start);
            }
            if (!gdead) lds_barrier();
        });
        // ---- LQ = LLRin + sum (:126) for the own entries
        if (!FIRST && active) {
            if constexpr (SUPD) {
                // every own entry read before the first add: one LDS round trip, not KH - 1
                T xo[KH];
#pragma unroll
                for (int jj = 0; jj < KH; ++jj) xo[jj] = jj == 0 ? S : at((uint32_t)(jcol(jj) * kFrColB) + sb);
#pragma unroll
                for (int jj = 0; jj < KH; ++jj) {
                    const int j = jcol(jj);
                    at((uint32_t)(j * kFrColB) + sb) = (j < pc ? T(0) : lf[jj]) + xo[jj];   // punctured columns: LLR 0 (:43)
                }
            } else {
#pragma unroll
                for (int jj = 0; jj < KH; ++jj) {
                    const int j = jcol(jj);
                    lds_T& x = at((uint32_t)(j * kFrColB) + sb);
                    x = (j < pc ? T(0) : lf[jj]) + (jj == 0 ? S : x);   // punctured columns: LLR 0 (:43)
                }
            }
        }
        if (!FIRST && t == 0) *flagA = 0;   // read before the phase-B barriers
        if constexpr (!FIRST) skipA = false;
        pre = true;   // (PRE) a trip that follows finds its cold start issued above
        if constexpr (FUSED) {
            // the loop's first trip begins with the barrier (its phase A is done above)
            if (!active) break;
        } else if constexpr (SBAR) {
            // `active` is workgroup-uniform here: every thread starts with it set and clears it
            // on the same test of the same LDS word (*flagI, read after phase A's barrier and
            // not written again before the next barrier: flagA's reset above comes after at
            // least one phase-B barrier, the peeled iteration's flag word is never reset).  So a
            // vote through LDS (block_any) would decide nothing: a plain barrier orders the LQ
            // update and the flag reset before the next trip, and every thread leaves alike.
            lds_barrier();
            if (!active) break;
        } else {
            if (!block_any(active)) break;
        }
    }
