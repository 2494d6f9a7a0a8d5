// libgpf_pairs.hip -- the kernels of the pairwise smoother per block (gpf_k_block_smooth.hpp, the walk it shares with k_block_smooth; gpf.h
// gpf_block_smooth_pairs, whose host side is in libgpf_store.hip).  A translation unit of their own, for the reason libgpf_smooth.hip is one: fifteen more
// instantiations of the block family's one compute-heavy walk, and every other unit's device code stays what it was (tools/isa_diff.py;
// profiles/block_pairs.md).
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M>
static void launch_block_pairs_model(gpf_filter* h, const PairArgs& a, const AncArgs& x)
{
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_smooth_pairs<M, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, a, x);
    });
}
void launch_block_pairs(gpf_filter* h, const PairArgs& a, const AncArgs& x)
{
    DISPATCH_MODEL(h, (launch_block_pairs_model<MM>(h, a, x)));
}

} // namespace gpfh
