// faster_sstate.inc — SStateHMM of the "--faster" model (reference Faster.cpp:253-576) up to the backtrack: emissions, the two sweeps towards
// bMid (both back-pointer encodings), the NS = 4/8/12/16 dispatch and the join at bMid.  ONE copy of the text, included in the body of
// dd_faster_kernel and of dd_faster_long_kernel (see faster_model.h for why it is a fragment and not a function).
// Reads the includer's locals: P (read_mqidx), T, rr, rd, qt, shHap, srt, bc, bt (LDS in one kernel, an HBM tile in the other), hlen, L, bMid,
// l16, relMine, act, Smax, l1mE, lE, NIf, IIf, hqOn, hqOff.  Defines: ll (the pair's log-likelihood) and xH (the state the backtrack starts
// from: diagonal | 16 if inserted); aN, aI, leftN, leftI, code0, code1, wI, emis, passes are its own.
            const int code0 = l16, code1 = l16 | 16;
            const int wI = 32 - __clz(l16 + 1);          // bits of the inserted-state field of bt_right: values 0..own+1

            // ---------------- SStateHMM (:253-576) ----------------
            auto emis = [&](int r, double &LM, double &ob) {            // logMatch[r] and obs[r][own diagonal] (:286-296)
                const unsigned v = rd[r];
                const double2 q = qt[v >> 8];
                const int hp = relMine + r;
                LM = q.x;
                ob = (hp >= 0 && hp < hlen && (unsigned)shHap[hp] != (v & 0xFFu)) ? q.y : q.x;
            };
            // Transition terms between every source diagonal cs and this lane's diagonal (:339-352) are loop constants.
            // A term that does not apply to this lane (wrong side of the diagonal order) is -inf, so the candidate it
            // produces is -inf and can never pass `nv > cur + EPS`: no lane masks in the inner loops.
            // Sources beyond the pair's S publish -inf, so the source loops may run to the next multiple of 4 of the
            // wave's largest S: four fully unrolled instances, no per-source bounds checks.
            double aN = 0.0, aI = 0.0;                  // previous base's values of this diagonal (0 at the read end)
            double leftN = 0.0, leftI = 0.0;
            auto passes = [&](auto nsc) {
                constexpr int NS = decltype(nsc)::value;
                int lv = l16;                               // opaque copy: keeps the per-source selects below from being hoisted
                asm volatile("" : "+v"(lv));                // out of the read loop as 2 x 16 spilled lane constants
            // from left to bMid (:373-416)
            {
                double tA[NS], tB[NS];
                int dL[NS];
#pragma unroll
                for (int cs = 0; cs < NS; cs++) {
                    const int df = srt[cs] - relMine;
                    const double trI = (fabs((double)df) - 1.0) * IIf;
                    tA[cs] = (cs < lv) ? trI + lE : (cs == lv ? l1mE : FNEG_INF);   // on-diagonal source cs <= own (:380-384)
                    tB[cs] = (cs > lv) ? trI : FNEG_INF;                              // inserted source cs > own (:404-411)
                    dL[cs] = (cs > lv) ? df : 0x7fffffff;                             // its condition relPos[cs]-r >= relPos[ns]
                    asm volatile("" : "+v"(tA[cs]), "+v"(tB[cs]), "+v"(dL[cs]));           // keep them as plain register constants
                }
                const int rows = gmax4(bMid);
                double LMn = 0.0, obn = 0.0;
                if (act && bMid > 0) emis(0, LMn, obn);
                for (int r = 0; r < rows; r++) {
                    const bool rowact = act && r < bMid;
                    const double LM = LMn, ob = obn;
                    const double pvOwn = ob + aN;
                    bc[l16] = rowact ? make_double2(pvOwn, aI) : make_double2(FNEG_INF, FNEG_INF);
                    wave_sync();
                    if (act && r + 1 < bMid) emis(r + 1, LMn, obn);
                    double curN = -1000.0, curI = -1000.0;
                    int bpN = 0, bpI = 32;                                      // untouched = the reference's bt 0: on-diagonal state of diagonal 0
#pragma unroll
                    for (int cs = 0; cs < NS; cs++) {
                        {
                            const double2 s = bc[cs];
                            const double vA = s.x + tA[cs];
                            const double vB = ((LM + tB[cs]) + lE) + s.y;
                            FOLD(curN, bpN, fmax(vA, vB), cs, dL[cs] >= r);
                        }
                    }
                    FOLD(curI, bpI, pvOwn + NIf, code0, true);                   // (:387-391)
                    FOLD(curI, bpI, (LM + IIf) + aI, code1, true);               // (:396-400)
                    if (rowact) {
                        bt[r * 16 + l16] = (unsigned char)(bpN | (bpI & 48));   // bt_left: bits 0-3 source diagonal of the on-diagonal state (a source above the own diagonal is its inserted state); bit 4: the inserted state came from itself, bit 5: it was never set
                        aN = curN; aI = curI;
                    }
                    wave_sync();
                }
            }
            leftN = aN; leftI = aI;                     // alpha[bMid-1] (0 if bMid == 0)
            // from right to bMid (:422-466)
            aN = 0.0; aI = 0.0;
            {
                double tD[NS], tA[NS];
                int dR[NS];
#pragma unroll
                for (int cs = 0; cs < NS; cs++) {
                    const int df = srt[cs] - relMine;
                    const double trI = (fabs((double)df) - 1.0) * IIf;
                    tD[cs] = (cs < lv) ? trI : FNEG_INF;                  // into the inserted state of a higher diagonal (:453-461)
                    tA[cs] = (cs > lv) ? trI + lE : FNEG_INF;             // on-diagonal source cs > own (:427-431); own: below
                    dR[cs] = df;                                           // condition relPos[cs] > relPos[ns]-r
                    asm volatile("" : "+v"(tD[cs]), "+v"(tA[cs]), "+v"(dR[cs]));
                }
                const int rows = gmax4(L - 1 - bMid);
                double LMn = 0.0, obn = 0.0;
                if (act && bMid < L - 1) emis(L - 1, LMn, obn);
                for (int k = 0; k < rows; k++) {
                    const int r = L - 1 - k;
                    const bool rowact = act && r > bMid;
                    const double LM = LMn, ob = obn;
                    bc[l16] = rowact ? make_double2(ob, aN) : make_double2(FNEG_INF, 0.0);
                    wave_sync();
                    if (act && r - 1 > bMid) emis(r - 1, LMn, obn);
                    double curN = -1000.0, curI = -1000.0;
                    int bpN = -1, bpI = -1;                                     // untouched = the reference's bt 0
                    FOLD(curN, bpN, (ob + aN) + l1mE, code0, true);              // own diagonal (:427-431)
                    FOLD(curN, bpN, (LM + lE) + aI, code1, true);                // (:436-438)
#pragma unroll
                    for (int cs = 0; cs < NS; cs++) {
                        {
                            const double2 s = bc[cs];
                            const double vD = ((s.x + NIf) + tD[cs]) + s.y;
                            const double vA = (s.x + s.y) + tA[cs];
                            FOLD(curI, bpI, vD, cs, dR[cs] > -r);
                            FOLD(curN, bpN, vA, cs, true);
                        }
                    }
                    FOLD(curI, bpI, (LM + IIf) + aI, code1, true);               // (:443-447)
                    if (rowact) {
                        // bt_right: two variable-width fields (widths depend on the diagonal, 8 bits in total at most):
                        // low wI bits, inserted state: 0 never set, 1 itself, 2+cs on-diagonal source cs < own;
                        // the rest, on-diagonal state: 0 never set, 1 own inserted state, 2+(cs-own) on-diagonal source cs >= own
                        const int iIdx = bpI < 0 ? 0 : ((bpI & 16) ? 1 : bpI + 2);
                        const int nIdx = bpN < 0 ? 0 : ((bpN & 16) ? 1 : bpN - l16 + 2);
                        bt[r * 16 + l16] = (unsigned char)(iIdx | (nIdx << wI));
                        aN = curN; aI = curI;
                    }
                    wave_sync();
                }
            }
            };
            if (Smax <= 4) passes(std::integral_constant<int, 4>());
            else if (Smax <= 8) passes(std::integral_constant<int, 8>());
            else if (Smax <= 12) passes(std::integral_constant<int, 12>());
            else passes(std::integral_constant<int, 16>());
            // join at bMid (:469-538): plain '>' maxima over x = ins*S + y
            double ll = FNEG_INF;
            int xH = 0;
            {
                double vN = FNEG_INF, vI = FNEG_INF, hN = FNEG_INF, hI = FNEG_INF;
                if (act) {
                    const int mqi = P.read_mqidx[rr];
                    const double lOn = T[T_MAPQF + 2 * mqi], lOff = T[T_MAPQF + 2 * mqi + 1];
                    double LM, ob;
                    emis(bMid, LM, ob);
                    const int hp = relMine + bMid;
                    const bool on = hp >= 0 && hp < hlen;
                    const bool hasR = bMid < L - 1, hasL = bMid > 0;
                    vN = ob + ((on ? lOn : lOff) + l1mE);
                    vI = LM + ((on ? lOn : lOff) + lE);
                    hN = ob + ((on ? hqOn : hqOff) + l1mE);
                    hI = LM + ((on ? hqOn : hqOff) + lE);
                    if (hasR) { vN += aN; vI += aI; hN += aN; hI += aI; }
                    if (hasL) { vN += leftN; vI += leftI; hN += leftN; hI += leftI; }
                }
                ll = vN > vI ? vN : vI;
                double mh = hI > hN ? hI : hN;                       // first maximum: the on-diagonal state wins a tie
                int mx = hI > hN ? 16 + l16 : l16;                   // order key: ins*16 + diagonal (same order as ins*S + y)
#pragma unroll
                for (int off = 8; off >= 1; off >>= 1) {
                    const double oll = __shfl_xor(ll, off, 16), omh = __shfl_xor(mh, off, 16);
                    const int omx = __shfl_xor(mx, off, 16);
                    ll = oll > ll ? oll : ll;
                    const bool tk = omh > mh || (omh == mh && omx < mx);
                    mh = tk ? omh : mh;
                    mx = tk ? omx : mx;
                }
                xH = (mh == FNEG_INF) ? 0 : mx;                      // nothing exceeded -inf: xmax stays 0 (:508)
            }
