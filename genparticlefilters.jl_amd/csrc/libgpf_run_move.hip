// libgpf_run_move.hip -- the kernels of the whole series per block with the rejuvenation moves inside (gpf_k_block_run_move.hpp; gpf.h
// gpf_run_blocks_rejuvenate, whose host side is in libgpf_blocks.hip).  A translation unit of their own, for the reason libgpf_run.hip is one: ninety
// instantiations -- each holds a model's sampler three times over beside a block resampler -- and every other unit's device code stays what it was
// (tools/isa_diff.py), k_block_run and the loop's kernels among them.
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M, int METHOD, bool REWEIGHT>
static void launch_block_run_move_as(gpf_filter* h, const RunMoveArgs& a)
{
    constexpr int Wc = row_width(Model<M>::D, true);             // 2 (sv1), 4 (the 2-D models) or 8 (bearings4)
    team_dispatch(a.r.nb, a.r.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_run_move<M, Wc, METHOD, REWEIGHT, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, a);
    });
}
void launch_block_run_move(gpf_filter* h, const RunMoveArgs& a, int method, bool reweight)
{
    bool_dispatch(reweight, [&](auto RW) {
        if (method == 0)      { DISPATCH_MODEL(h, (launch_block_run_move_as<MM, 0, RW>(h, a))); }
        else if (method == 1) { DISPATCH_MODEL(h, (launch_block_run_move_as<MM, 1, RW>(h, a))); }
        else                  { DISPATCH_MODEL(h, (launch_block_run_move_as<MM, 2, RW>(h, a))); }
    });
}

} // namespace gpfh
