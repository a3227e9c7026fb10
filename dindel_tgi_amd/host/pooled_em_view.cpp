// pooled_em_view.cpp — pooled_em.hpp's PooledWindow from the lazy view of a batch's records (and filterHaplotypes on it).
#include "pooled_em.hpp"

namespace dindel {

void pooledWindowOf(const std::vector<Haplotype> &haps, const std::vector<Read> &reads, const WindowLikelihoods &liks, const DiploidParameters &params,
                    PooledWindow &win)
{
    win = PooledWindow();
    win.nh = haps.size(); win.nr = reads.size();
    win.ll.resize(win.nh * win.nr); win.offHap.resize(win.nh * win.nr);
    for (size_t h = 0; h < win.nh; h++) {
        const WindowLikelihoods::Rows rows = liks.rows(h);
        for (size_t r = 0; r < win.nr; r++) { win.ll[h * win.nr + r] = rows.ll[r]; win.offHap[h * win.nr + r] = rows.offHap[r]; }
    }
    win.filtered.assign(win.nh, 0);
    filterHaplotypes(haps, reads, liks, win.filtered, win.varCoverage, params.filterHaplotypes);      // always called (DInDel.cpp:2149)
    win.covered = [liks](size_t h, size_t r, int pos, bool snp) { return liks.coveredAt(h, r, liks.varSlot(h, pos, snp)); };
}

} // namespace dindel
