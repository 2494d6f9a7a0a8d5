// libgpf_run_hist.hip -- the kernels of the whole series per block that records the block-wise trajectory store (k_block_series<.., RunHist<WEIGHTS>>, gpf_k_block_run.hpp; gpf.h
// gpf_run_blocks_history, whose host side is in libgpf_blocks.hip).  A translation unit of their own, for the reason libgpf_run.hip is one: ninety
// instantiations -- the plain run's forty-five with and without the store's weight records -- and every other unit's device code stays what it was
// (tools/isa_diff.py), the plain run's and the loop's kernels among them.
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M, int METHOD, bool WEIGHTS>
static void launch_block_run_hist_as(gpf_filter* h, const RunArgs& a, const RunHistArgs& hs)
{
    constexpr int Wc = row_width(Model<M>::D, false);            // (a keep_prev state is refused, as by gpf_run_blocks)
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_series<M, Wc, METHOD, TEAM, ITEMS, RunHist<WEIGHTS>>), grid, dim3(BLOCK), 0, h->stream, a, RunHist<WEIGHTS>{hs});
    });
}
void launch_block_run_hist(gpf_filter* h, const RunArgs& a, const RunHistArgs& hs, int method, bool weights)
{
    bool_dispatch(weights, [&](auto WT) {
        if (method == 0)      { DISPATCH_MODEL(h, (launch_block_run_hist_as<MM, 0, WT>(h, a, hs))); }
        else if (method == 1) { DISPATCH_MODEL(h, (launch_block_run_hist_as<MM, 1, WT>(h, a, hs))); }
        else                  { DISPATCH_MODEL(h, (launch_block_run_hist_as<MM, 2, WT>(h, a, hs))); }
    });
}

} // namespace gpfh
