// cxl-speckv_amd/csrc/codec_launch_shape.hpp -- the launch shape of the block codec (k_fetch_decompress*, k_compress) as ONE pure host
// function: how many workgroups a launch of n blocks gets, how many blocks a wave owns and how far apart they lie.  launch_decompress /
// launch_compress (kernels.hip) size every launch with it and speckv_ext_codec_launch_shape (c_api.cpp) exports the same body under the
// tuning in force, so the launchers, the export and the tests agree by construction.  Plain C++17, no HIP.
#pragma once
#include <cstdint>

namespace speckv {

constexpr uint32_t kCodecWgsPerCuDefault = 256;           // tuning key wgs_per_cu = 0

struct CodecLaunchShape {
    uint32_t grid;        // workgroups of `waves` waves
    uint64_t per_wave;    // blocks a wave owns (1: the plain form)
    uint64_t wave_step;   // per_wave > 1: distance of a wave's blocks (grid x waves: one per round), 0: they are consecutive
};

// One block per wave up to per_cu workgroups per CU (short-lived waves even out the tail); beyond that every wave takes the same
// number of blocks (per_wave) so that no round runs half empty.
// (A capped grid-stride loop: 655 360 blocks over 65 536 workgroups = 2.5 rounds, last one half empty: 0.73 of HBM
// peak; balanced 0.77-0.80.  Measured with profiles/tools/footprint.py, profiles/r02_footprint.md.)
// Multi-round launches: a wave's blocks are one grid apart (round r covers blocks [r*G, (r+1)*G) like a launch of its
// own) unless `consecutive`.  Measured against `per_wave` consecutive blocks per wave on the same device (SPECKV_ROUNDS=consecutive):
// 0.775 / 0.772 / 0.770 of HBM peak vs 0.753 / 0.69 / 0.657 at 4 / 5 / 20 GiB of pool + destination.
// The kernels walk the shape as: gw = workgroup x waves + wave; strided  i = gw, gw + wave_step, ... while i < n;
// consecutive  i in [gw x per_wave, min(gw x per_wave + per_wave, n)).  Every block of [0, n) belongs to exactly one wave, also
// for a smaller n read on the device (CodecArgs::n_dev).  n == 0: a grid of one workgroup that finds nothing to do.
inline CodecLaunchShape codec_launch_shape(uint64_t n, uint32_t n_cus, int32_t wgs_per_cu, bool consecutive, uint32_t waves)
{
    const uint64_t per_cu = wgs_per_cu > 0 ? static_cast<uint64_t>(wgs_per_cu) : kCodecWgsPerCuDefault;
    const uint64_t want = (n + waves - 1) / waves;
    const uint64_t cap = static_cast<uint64_t>(n_cus) * per_cu * (4 / waves);
    if (want <= cap) return {static_cast<uint32_t>(want ? want : 1), 1, 0};
    const uint64_t rounds = (want + cap - 1) / cap;
    const uint32_t grid = static_cast<uint32_t>((want + rounds - 1) / rounds);
    return {grid, rounds, consecutive ? 0 : static_cast<uint64_t>(grid) * waves};
}

} // namespace speckv
