// cxl-speckv_amd/csrc/fetch_sweep.hpp -- the direction in which a fetch_range launch walks its blocks, as ONE pure host function.
// Engine::fetch_range (engine_io.cpp) decides every kernel-path launch with it and speckv_ext_fetch_sweep_next (c_api.cpp) exports the
// same body, so the engine, the export and the tests agree by construction.  Plain C++17, no HIP.
//
// Why a direction at all: a call that sweeps more than the Infinity Cache holds (256 MiB), repeated over the same range in ascending
// order, is the worst case of a least-recently-used cache -- when block 0 comes round again everything behind it has passed through,
// and every access misses.  What the previous sweep touched LAST is still on die when the next one starts; a sweep that starts there
// and walks the other way overwrites destination lines that were never written back -- provided the previous sweep's stores allocated
// in the cache, which non-temporal stores (the codec's default: the faster ones for an image nobody touches again soon) do not.  So the
// rule decides two things for a launch: its direction (CodecArgs::descending) and whether its stores are plain (CodecArgs::keep_stores).
// Measured (profiles/sweep_direction.txt, 131 072 blocks, one process): alternation with non-temporal stores gains nothing; plain
// stores without alternation lose 4 % (8 % as a build-wide policy); both together gain 10 %.  Non-temporal record loads stay: plain ones compete with the
// destination for the cache and the gain shrinks.  No work is skipped and nothing is cached in software: every block is decoded on
// every call, only the order and the store marking change.  A caller that fetches many small ranges with the whole pool between two
// uses of one range never repeats its previous range: its launches stay ascending and non-temporal, it gains nothing and loses nothing.
#pragma once
#include <cstdint>

namespace speckv {

// the previous kernel-path fetch_range of an allocation (Allocation::sweep); cleared wherever the handle's row is freed or recycled
struct FetchSweepState {
    uint64_t first = 0;
    uint64_t n = 0;
    uint32_t descending = 0;
    uint32_t valid = 0;
};

struct FetchSweepNext {
    uint32_t descending;      // this call's direction
    uint32_t keep_stores;     // this call's stores are plain: the sweep after it finds them on die
    FetchSweepState state;    // what the allocation remembers after it
};

// tuning key fetch_sweep
constexpr int32_t kFetchSweepNever = 0, kFetchSweepAlternate = 1, kFetchSweepAlways = 2, kFetchSweepAlternateNt = 3;
// The rule's upper bound: what a sweep saves is at most the cache's 256 MiB, what plain stores cost grows with the range (5 % of it
// without alternation).  Measured gain of mode 1 over mode 0 at 65 536 / 131 072 / 262 144 / 393 216 blocks: 5.9 / 9.5 / 4.9 / 2.3 %;
// at 524 288 blocks (4 GiB of records and destination) it LOSES 1.4 %.  Ranges beyond the largest size that gained stay as they were.
constexpr uint64_t kFetchSweepMaxBlocks = 393216;

// mode 1: the same (first, n) as the allocation's previous fetch, n <= kFetchSweepMaxBlocks -- the opposite direction, plain stores.  Anything else -- the first
// fetch, another range -- ascending, non-temporal stores.  A capturing stream: ascending, non-temporal and the state as it was (a
// replayed graph cannot alternate).  mode 0: always ascending and non-temporal; mode 2: always descending with plain stores (tests and
// measurements force the other form with it); mode 3: the directions of mode 1 with non-temporal stores (measurements: what the
// alternation is worth by itself).  Every mode records the call like mode 1.
// (The copy-engine path never comes here: it stays ascending and leaves the state alone.)
inline FetchSweepNext fetch_sweep_next(const FetchSweepState& prev, uint64_t first, uint64_t n, bool capturing, int32_t mode)
{
    if (capturing) return {0u, 0u, prev};
    const bool repeat = prev.valid && prev.first == first && prev.n == n;
    uint32_t down = 0, keep = 0;
    if (mode == kFetchSweepAlways) down = keep = 1;
    else if (mode == kFetchSweepAlternateNt ? repeat : (mode == kFetchSweepAlternate && repeat && n <= kFetchSweepMaxBlocks)) {
        down = prev.descending ? 0u : 1u;
        keep = mode == kFetchSweepAlternate ? 1u : 0u;
    }
    return {down, keep, FetchSweepState{first, n, down, 1u}};
}

} // namespace speckv
