// libgpf_gibbs.hip -- the kernels of the particle Gibbs chain per block in one launch (k_block_gibbs, gpf_k_block_gibbs.hpp; gpf.h gpf_gibbs_blocks, whose host
// side is in libgpf_blocks.hip).  A translation unit of their own, for the reason libgpf_sweep.hip is one: sixty more instantiations -- each holds a
// model's sampler twice, for the initial step and the propagate, beside a block resampler and its transition density -- next to the sweep's would change
// their register allocation; here every other unit's device code stays what it was (tools/isa_diff.py), the sweep's kernels among them.
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M, bool AS, bool BACK>
static void launch_block_gibbs_as(gpf_filter* h, const GibbsArgs& a)
{
    constexpr int Wc = row_width(Model<M>::D, false);            // (a keep_prev state is refused: x_{t-1} serves only the moves)
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_gibbs<M, Wc, AS, TEAM, ITEMS, BACK>), grid, dim3(BLOCK), 0, h->stream, a);
    });
}
void launch_block_gibbs(gpf_filter* h, const GibbsArgs& a, bool ancestor_sampling, bool backward)
{
    if (backward) {
        if (ancestor_sampling) { DISPATCH_MODEL(h, (launch_block_gibbs_as<MM, true, true>(h, a))); }
        else                   { DISPATCH_MODEL(h, (launch_block_gibbs_as<MM, false, true>(h, a))); }
    } else {
        if (ancestor_sampling) { DISPATCH_MODEL(h, (launch_block_gibbs_as<MM, true, false>(h, a))); }
        else                   { DISPATCH_MODEL(h, (launch_block_gibbs_as<MM, false, false>(h, a))); }
    }
}

} // namespace gpfh
