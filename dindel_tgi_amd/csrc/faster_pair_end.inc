// faster_pair_end.inc — the end of a pair in the "--faster" model, after the kernel has mapped the states (st), written hpos and gathered each
// lane's firstB / lastB: the firstBase / lastBase reduction, var_covered, the filterHaplotypes coverage test (var_fcov) and the final store
// of ll / status / firstBase / lastBase.  ONE copy of the text, included in the body of dd_faster_kernel and of dd_faster_long_kernel (see
// faster_model.h for why it is a fragment and not a function).
// Reads the includer's locals: P, w, g, h0, R, ri, nv, pair, good, l16, hlen, L, ll, firstB, lastB, st, rd, shHap, bm; defines vb.
// The includer defines FAST_ST_VISIBLE(): what it takes for a lane to read the st entries the other 15 lanes wrote (nothing where st is
// LDS behind a wave_sync, a tile_sync where it is HBM).
#pragma unroll
            for (int off = 8; off >= 1; off >>= 1) {
                const int f = __shfl_xor(firstB, off, 16), l2 = __shfl_xor(lastB, off, 16);
                firstB = f < firstB ? f : firstB;
                lastB = l2 > lastB ? l2 : lastB;
            }
            if (firstB == 0x7fffffff) firstB = -1;
            const int64_t vb = (nv > 0) ? P.win_varcov_off[w] + (int64_t)(P.hap_var_off[g] - P.hap_var_off[h0]) * R + (int64_t)ri * nv : 0;
            if (P.out.var_covered && nv > 0 && good) {
                for (int i = l16; i < nv; i += 16) {
                    const int sR = P.hap_var[2 * (P.hap_var_off[g] + i)], eR = P.hap_var[2 * (P.hap_var_off[g] + i) + 1];
                    P.out.var_covered[vb + i] = (firstB + P.padCover <= sR && lastB - P.padCover >= eR) ? 1 : 0;
                }
            }
            // DetInDel::filterHaplotypes' per-read test (DInDel.cpp:1951-2054): this model leaves numIndels = 0 and
            // offHapHMQ = false, so every read is selected, and its hpos may skip or repeat haplotype bases: the
            // covered set is marked base by base (one bit per haplotype base).  Sentinel hpos values (< 0) never cover anything:
            // an interval reaching below haplotype base 0 is never covered (the reference indexes the sequence with them there).
            if (P.out.var_fcov && P.hap_var_flank && nv > 0) {
                FAST_ST_VISIBLE();                                   // the includer's: the other lanes' mapped states (st) can be read
                for (int i = 0; i < nv; i++) {
                    const int32_t *fl = P.hap_var_flank + 3 * (size_t)(P.hap_var_off[g] + i);
                    const int left = fl[0] - P.padCover, right = fl[1] + P.padCover, kind = fl[2];
                    int cov = 0;
                    if (kind != 0 && right >= left) {
                        wave_sync();
                        for (int x = l16; x < (hlen + 31) / 32; x += 16) bm[x] = 0;
                        wave_sync();
                        int nmm = 0;
                        for (int b = l16; b < L; b += 16) {
                            const int s2 = st[b];
                            if (s2 >= 1 && s2 <= hlen) {
                                const int hb = s2 - 1;
                                if (hb >= left && hb <= right) {
                                    atomicOr(&bm[hb >> 5], 1 << (hb & 31));
                                    const unsigned hc = shHap[hb];
                                    nmm += ((rd[b] & 0xFFu) != hc && (kind == 2 || hc != 'N')) ? 1 : 0;   // 'N' exempt for DEL (:1992)
                                }
                            }
                        }
                        wave_sync();
                        int csize = 0;
                        const int lo = left > 0 ? left : 0, hi = right < hlen - 1 ? right : hlen - 1;
                        for (int x = lo + l16; x <= hi; x += 16) csize += (bm[x >> 5] >> (x & 31)) & 1;
#pragma unroll
                        for (int off = 8; off >= 1; off >>= 1) {
                            nmm += __shfl_xor(nmm, off, 16);
                            csize += __shfl_xor(csize, off, 16);
                        }
                        cov = (csize >= right - left + 1 && nmm <= P.maxMismatch) ? 1 : 0;
                    }
                    if (l16 == 0 && good) P.out.var_fcov[vb + i] = (uint8_t)cov;
                }
            }
            if (l16 == 0 && good) {
                P.out.ll[pair] = ll;
                P.out.status[pair] = DD_PAIR_OK;             // computeLikelihoodsFaster has no ll checks
                if (P.out.firstBase) P.out.firstBase[pair] = (int16_t)firstB;
                if (P.out.lastBase) P.out.lastBase[pair] = (int16_t)lastB;
            }
