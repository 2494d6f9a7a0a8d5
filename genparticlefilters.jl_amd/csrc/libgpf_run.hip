// libgpf_run.hip -- the kernels of the whole series per block in one launch (gpf_k_block_run.hpp; gpf.h gpf_run_blocks, whose host side is in
// libgpf_blocks.hip).  A translation unit of their own, for the reason libgpf_smooth.hip is one: forty-five more instantiations -- each holds a model's
// sampler beside a block resampler -- next to the other block kernels would change their register allocation; here every other unit's device code stays
// what it was (tools/isa_diff.py), the loop's kernels among them.
#include "gpf_host.hpp"

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M, int METHOD>
static void launch_block_run_as(gpf_filter* h, const RunArgs& a)
{
    constexpr int Wc = row_width(Model<M>::D, false);            // (a keep_prev state is refused: x_{t-1} serves only the moves)
    team_dispatch(a.nb, a.nblocks, [&](auto TEAM, auto ITEMS, dim3 grid) {
        GPF_LAUNCH((k_block_run<M, Wc, METHOD, TEAM, ITEMS>), grid, dim3(BLOCK), 0, h->stream, a);
    });
}
void launch_block_run(gpf_filter* h, const RunArgs& a, int method)
{
    if (method == 0)      { DISPATCH_MODEL(h, (launch_block_run_as<MM, 0>(h, a))); }
    else if (method == 1) { DISPATCH_MODEL(h, (launch_block_run_as<MM, 1>(h, a))); }
    else                  { DISPATCH_MODEL(h, (launch_block_run_as<MM, 2>(h, a))); }
}

} // namespace gpfh
