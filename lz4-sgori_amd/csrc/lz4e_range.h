// lz4e_range.h -- the validity test of a range read's request, shared by the
// range kernels (lz4e_pack.hip) and the kernels that wrap them for the
// verified range read (lz4e_crc.hip): one text, so the two calls cannot come
// to disagree on what "invalid" means.
#pragma once

#include <stdint.h>

#include "lz4e_gpu.h"
#include "lz4e_wave.h"

namespace lz4e {
namespace {

struct RangeReq {
    uint32_t entry;
    bool valid;  // the entry exists, its kind is known, its length and the range are not negative
};
LZ4E_DEV RangeReq range_req(const uint32_t* sel, const int32_t* lo, const int32_t* len, const int32_t* pk_len,
                            const uint8_t* pk_kind, uint32_t nentries, uint64_t j) {
    const uint32_t e = sel ? sel[j] : (uint32_t)j;
    bool ok = e < nentries && lo[j] >= 0 && len[j] >= 0;
    if (ok) ok = (pk_kind[e] == kPackFrame || pk_kind[e] == kPackRaw) && pk_len[e] >= 0;
    return RangeReq{e, ok};
}

}  // namespace
}  // namespace lz4e
