// libgpf_pmmh.hip -- the kernels of the particle-marginal MH move per block in one launch (k_block_pmmh, gpf_k_block_pmmh.hpp; gpf.h gpf_pmmh_blocks, whose host
// side is in libgpf_blocks.hip).  A translation unit of their own, for the reason libgpf_run.hip is one: forty-five more instantiations -- each holds a
// model's sampler twice, for the initial step and the propagate, beside a block resampler -- next to the other block kernels would change their register
// allocation; here every other unit's device code stays what it was (tools/isa_diff.py).
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M, int METHOD>
static void launch_block_pmmh_as(gpf_filter* h, const PmmhArgs& a)
{
    constexpr int Wc = row_width(Model<M>::D, false);            // (a keep_prev state is refused, as by gpf_run_blocks)
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_pmmh<M, Wc, METHOD, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, a);
    });
}
void launch_block_pmmh(gpf_filter* h, const PmmhArgs& a, int method)
{
    if (method == 0)      { DISPATCH_MODEL(h, (launch_block_pmmh_as<MM, 0>(h, a))); }
    else if (method == 1) { DISPATCH_MODEL(h, (launch_block_pmmh_as<MM, 1>(h, a))); }
    else                  { DISPATCH_MODEL(h, (launch_block_pmmh_as<MM, 2>(h, a))); }
}
// does a block of this size keep the proposal filter in LDS (pmmh_in_lds of the team shape team_dispatch gives it), W the filter's row width
bool block_pmmh_in_lds(int64_t block_size, int W)
{
    bool r = false;
    team_dispatch(block_size, 1, [&](auto, auto ITEMS, dim3) { r = W == 2 ? pmmh_in_lds<2, ITEMS>() : pmmh_in_lds<4, ITEMS>(); });
    return r;
}

} // namespace gpfh
