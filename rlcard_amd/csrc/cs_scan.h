// cs_scan.h -- the prefix sum of the launchers (hipcub::DeviceScan): size query, scratch, scan in one call.
#pragma once
#include <hipcub/hipcub.hpp>
#include "cs_devbuf.h"

namespace cs {

template <bool INCLUSIVE, class In, class Out, class N>
hipError_t scan_sum_run(void* tmp, size_t& bytes, In in, Out out, N count, hipStream_t s)
{
    if constexpr (INCLUSIVE) return hipcub::DeviceScan::InclusiveSum(tmp, bytes, in, out, count, s);
    else return hipcub::DeviceScan::ExclusiveSum(tmp, bytes, in, out, count, s);
}

// the scratch is `grow`, grown to what the scan asks for, or without one the `bytes` at `tmp`
template <bool INCLUSIVE, class In, class Out, class N>
hipError_t scan_sum_in(DevBuf* grow, void* tmp, size_t bytes, In in, Out out, N count, hipStream_t s)
{
    size_t need = 0;
    hipError_t e = scan_sum_run<INCLUSIVE>(nullptr, need, in, out, count, s);
    if (e == hipSuccess && grow) {
        e = grow->reserve(need);
        tmp = grow->p;
        bytes = grow->bytes;
    }
    if (e != hipSuccess) return e;
    if (need > bytes) return hipErrorInvalidValue;
    return scan_sum_run<INCLUSIVE>(tmp, need, in, out, count, s);
}

// out[0..count) = the exclusive (or inclusive) sum of in[0..count) on stream s, in scratch grown on demand
template <bool INCLUSIVE = false, class In, class Out, class N>
hipError_t scan_sum(DevBuf& tmp, In in, Out out, N count, hipStream_t s)
{
    return scan_sum_in<INCLUSIVE>(&tmp, nullptr, 0, in, out, count, s);
}

// the same in scratch the caller owns: `bytes` at `tmp`, which must hold what the scan asks for
template <bool INCLUSIVE = false, class In, class Out, class N>
hipError_t scan_sum(void* tmp, size_t bytes, In in, Out out, N count, hipStream_t s)
{
    return scan_sum_in<INCLUSIVE>(nullptr, tmp, bytes, in, out, count, s);
}

}  // namespace cs
