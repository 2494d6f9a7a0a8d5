// libgpf_map.hip -- the kernels of the most probable path per block (gpf_k_block_map.hpp; gpf.h gpf_block_map_path, whose host side is in libgpf_store.hip).
// A translation unit of their own, for the reason libgpf_smooth.hip is one: fifteen more instantiations beside the other block kernels would change their
// register allocation; here every other unit's device code stays what it was (tools/isa_diff.py).
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M>
static void launch_block_map_model(gpf_filter* h, const MapArgs& a, const AncArgs& x)
{
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_map<M, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, a, x);
    });
}
void launch_block_map(gpf_filter* h, const MapArgs& a, const AncArgs& x)
{
    DISPATCH_MODEL(h, (launch_block_map_model<MM>(h, a, x)));
}

} // namespace gpfh
