// cxl-speckv_amd/csrc/copy_records_device.hpp -- what the record-copy kernels share: k_copy_records (copy_records.hip, one allocation
// pair per descriptor) and k_copy_records_kv (copy_records_kv.hip, the split pool's two): the accesses and the scalar bookkeeping.
// Behind them the two halves of a record's copy as functions -- its bytes (copy_record_bytes) and its page-table entry with the scale
// table (copy_record_entry) -- which k_copy_records_kv calls once per format.  They are the text of k_copy_records' loop body;
// k_copy_records keeps that text inline, because calling these instead reschedules five of its six instances (47-53 instructions
// fewer, but not the instructions the unit is pinned to), so a change to either copy is made in both places.
#pragma once
#include "kernels.hpp"
#include "attend_device.hpp"         // u32x4

namespace speckv {
namespace {

constexpr uint32_t kCopyWaves = 4;
constexpr uint32_t kCopyWgsPerCu = 8;            // 32 waves per CU: the kernels need few registers and no LDS

typedef u32x4 __attribute__((address_space(1))) gc_u32x4;
__device__ __forceinline__ u32x4 cp_ld16(const uint8_t* p)
{
    return __builtin_nontemporal_load((const gc_u32x4*)(reinterpret_cast<uintptr_t>(p)));
}
__device__ __forceinline__ void cp_st16(uint8_t* p, u32x4 v)
{
    __builtin_nontemporal_store(v, (gc_u32x4*)(reinterpret_cast<uintptr_t>(p)));
}
template <typename T> __device__ __forceinline__ void cp_store(void* p, T v)
{
    typedef T __attribute__((address_space(1))) G;
    *(G*)(reinterpret_cast<uintptr_t>(p)) = v;
}
// a page-table entry read at an address all lanes share, kept in scalar registers
struct EntryWords { uint64_t addr; uint32_t len, scale_bits; };
__device__ __forceinline__ EntryWords cp_entry(const PageEntry* e)
{
    const u32x4 w = *(const gc_u32x4*)(reinterpret_cast<uintptr_t>(e));
    const uint32_t lo = __builtin_amdgcn_readfirstlane(w.x), hi = __builtin_amdgcn_readfirstlane(w.y);
    return EntryWords{(static_cast<uint64_t>(hi) << 32) | lo, static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(w.z)),
                      static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(w.w))};
}
__device__ __forceinline__ uint64_t cp_uniform(uint64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v)), hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// the longest record of a scheme: what a copy is cut to, so that entry words that are not a record length can never carry a store
// beyond the destination's slot (slots are at least this long: stride_for, engine_internal.hpp)
template <int SCHEME> constexpr uint32_t max_rec_bytes()
{
    return SCHEME == kInt8 || SCHEME == kFp8E4m3 ? kBlockElems : SCHEME == kInt4G32 ? kInt4RecBytes : SCHEME == kMxFp4 ? kMx4RecBytes : 2u * kBlockElems;
}

// The bytes of one record, source entry s to destination entry d, by one wave; returns the length the destination's entry gets.
template <int SCHEME>
__device__ __forceinline__ uint32_t copy_record_bytes(const EntryWords& s, const EntryWords& d, uint32_t lane)
{
    const uint8_t* src = reinterpret_cast<const uint8_t*>(s.addr);
    uint8_t* dst = reinterpret_cast<uint8_t*>(d.addr);
    constexpr uint32_t kMax = max_rec_bytes<SCHEME>();
    const uint32_t len = s.len < kMax ? s.len : kMax;
    if (len) {
        if (SCHEME == kMxFp4) {
            // tile-planar: the nibble row at the record's address, the 64 code bytes a slot-dependent distance behind it -- the
            // source's distance to read, the destination's own to write (PageEntry::scale holds it; it is not copied)
            const u32x4 nib = cp_ld16(src + 16u * lane);
            u32x4 code = {0u, 0u, 0u, 0u};
            if (lane < 4u) code = cp_ld16(src + s.scale_bits + 16u * lane);
            cp_st16(dst + 16u * lane, nib);
            if (lane < 4u) cp_st16(dst + d.scale_bits + 16u * lane, code);
        } else {
            // rounded up to 16 inside the slot: the encoder zero-pads a record's last 16-byte piece, slots and packed extents are
            // 128-byte aligned
            const uint32_t bytes = (len + 15u) & ~15u;
            u32x4 v[4];
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t b = 1024u * j + 16u * lane;
                if (1024u * j < kMax && b < bytes) v[j] = cp_ld16(src + b);
            }
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t b = 1024u * j + 16u * lane;
                if (1024u * j < kMax && b < bytes) cp_st16(dst + b, v[j]);
            }
        }
    } else if (d.len) {
        // a page never written replaces a record: the slot goes back to zero bytes, which is what the attention forms that
        // compute record addresses read for a page never written
        const u32x4 zero = {0u, 0u, 0u, 0u};
        if (SCHEME == kMxFp4) {
            cp_st16(dst + 16u * lane, zero);
            if (lane < 4u) cp_st16(dst + d.scale_bits + 16u * lane, zero);
        } else {
            const uint32_t bytes = ((d.len < kMax ? d.len : kMax) + 15u) & ~15u;
#pragma unroll
            for (uint32_t j = 0; j < 4u; ++j) {
                const uint32_t b = 1024u * j + 16u * lane;
                if (1024u * j < kMax && b < bytes) cp_st16(dst + b, zero);
            }
        }
    }
    return len;
}

// The destination's entry words for the record just copied, by lane 0; g (a CopyPair or CopyPairKV) names the scale table of the
// destination.  TAB false: an allocation that never has one (the V side of the split pool).
template <int SCHEME, bool TAB, class PAIR>
__device__ __forceinline__ void copy_record_entry(PageEntry* e, uint64_t page, uint32_t len, uint32_t scale_bits, const PAIR* g)
{
    cp_store<uint32_t>(&e->rec_bytes, len);
    if (SCHEME != kMxFp4) cp_store<uint32_t>(&e->scale, scale_bits);
    if (!TAB) return;
    // the block scale wherever k_compress leaves it (FP8 allocations with a layout), a page never written as
    // launch_build_scale_tab has it
    float* const scale_tab = g->scale_tab;
    if (scale_tab) {
        const uint32_t region_pages = g->region_pages, scale_run = g->scale_run;
        const uint32_t sc = len >= kBlockElems ? scale_bits : 0u;
        const uint32_t j = static_cast<uint32_t>(page % region_pages) & 15u;
        cp_store<uint32_t>(&scale_tab[page - j + attend_tile_slot(j)], sc);
        if (scale_run) cp_store<uint32_t>(scale_tab + scale_run_index(page, scale_run), sc);
    }
}

} // namespace
} // namespace speckv
