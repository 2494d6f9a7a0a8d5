// libgpf_smooth.hip -- the kernels of the marginal smoother per block (gpf_k_block_smooth.hpp; gpf.h gpf_block_smooth, whose host side is in libgpf_store.hip).
// A translation unit of their own: k_block_smooth is the one compute-heavy kernel of the block family (fifteen instantiations of 150-256 registers), and
// instantiated beside the other block kernels it changed their register allocation; here every other unit's device code stays what it was.
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M>
static void launch_block_smooth_model(gpf_filter* h, const SmoothArgs& a, const AncArgs& x)
{
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_smooth<M, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, a, x);
    });
}
void launch_block_smooth(gpf_filter* h, const SmoothArgs& a, const AncArgs& x)
{
    DISPATCH_MODEL(h, (launch_block_smooth_model<MM>(h, a, x)));
}

} // namespace gpfh
