// libgpf_sweep_back.hip -- the kernels of the conditional SMC sweep per block with a backward-simulation draw, in one launch (k_block_sweep<.., BACK = true>, gpf_k_block_sweep.hpp;
// gpf.h gpf_sweep_blocks_backward, whose host side is in libgpf_blocks.hip).  A translation unit of their own, for the reason libgpf_sweep.hip is one:
// thirty more instantiations -- each holds a model's sampler beside a block resampler and its transition density twice -- next to the sweep's would
// change their register allocation; here every other unit's device code stays what it was (tools/isa_diff.py), the sweep's kernels among them.
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M, bool AS>
static void launch_block_sweep_back_as(gpf_filter* h, const SweepArgs& a)
{
    constexpr int Wc = row_width(Model<M>::D, false);            // (a keep_prev state is refused: x_{t-1} serves only the moves)
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_sweep<M, Wc, AS, TEAM, ITEMS, true>), grid, dim3(BLOCK), 0, h->stream, a);
    });
}
void launch_block_sweep_back(gpf_filter* h, const SweepArgs& a, bool ancestor_sampling)
{
    if (ancestor_sampling) { DISPATCH_MODEL(h, (launch_block_sweep_back_as<MM, true>(h, a))); }
    else                   { DISPATCH_MODEL(h, (launch_block_sweep_back_as<MM, false>(h, a))); }
}

} // namespace gpfh
