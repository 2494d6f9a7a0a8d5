// libgpf_run_wide.hip -- the kernels of the whole series per block in one launch for blocks of 2049 .. 8192 particles (gpf_k_block_run_wide.hpp; gpf.h
// gpf_run_blocks_wide, whose host side is in libgpf_blocks.hip).  A translation unit of their own, for the reason libgpf_run.hip is one: fifteen more
// instantiations -- each holds a model's sampler beside a block resampler -- next to the other block kernels would change their register allocation;
// here every other unit's device code stays what it was (tools/isa_diff.py).
#include "gpf_host.hpp"

#include <atomic>

using namespace gpf;
using namespace gpfh;

namespace gpfh {

template <int M, int METHOD>
static gpf_status launch_block_run_wide_as(gpf_filter* h, const RunArgs& a)
{
    constexpr int Wc = row_width(Model<M>::D, false);            // (a keep_prev state is refused: x_{t-1} serves only the moves)
    const auto kernel = &k_block_run_wide<M, Wc, METHOD>;
    // the dynamic LDS of the largest block, allowed once per kernel and device (as libgpf_resample.hip allows its search kernels theirs)
    static std::atomic<uint64_t> allowed{0};
    const uint64_t bit = 1ull << (h->cfg.device & 63);
    if (!(allowed.load() & bit)) {
        HIP_TRY(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)wide_lds_bytes(METHOD, BLK_WIDE_MAX)));
        allowed.fetch_or(bit);
    }
    GPF_LAUNCH(kernel, dim3((unsigned)a.nblocks), dim3(WIDE), (unsigned)wide_lds_bytes(METHOD, a.nb), h->stream, a);
    return GPF_OK;
}
gpf_status launch_block_run_wide(gpf_filter* h, const RunArgs& a, int method)
{
    gpf_status s = GPF_OK;
    if (method == 0)      { DISPATCH_MODEL(h, (s = launch_block_run_wide_as<MM, 0>(h, a))); }
    else if (method == 1) { DISPATCH_MODEL(h, (s = launch_block_run_wide_as<MM, 1>(h, a))); }
    else                  { DISPATCH_MODEL(h, (s = launch_block_run_wide_as<MM, 2>(h, a))); }
    return s;
}

} // namespace gpfh
