// cxl-speckv_amd/csrc/engine_internal.hpp -- what the engine_*.cpp translation units share besides the class itself:
// error / logging macros, the device scope, small host helpers.  (engine.cpp was one file of 3 200 lines until round 4; it is
// now cut along its seams: engine.cpp pool, tiers, ring, access | engine_flush.cpp look-ahead, flush, predictor |
// engine_io.cpp write / read / bulk fetch | engine_attend.cpp fused-attention planning | engine_relocate.cpp migration,
// compaction.  No behaviour changed in the cut.)
#pragma once
#include "engine.hpp"
#include "placement.hpp"
#include "tuning.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace speckv {
namespace {

bool g_verbose = [] { const char* e = getenv("SPECKV_LOG"); return e && *e && *e != '0'; }();

#define SPECKV_ERR(...) do { fprintf(stderr, "[libcxlspeckv] " __VA_ARGS__); fputc('\n', stderr); } while (0)
#define SPECKV_LOGV(...) do { if (g_verbose) { fprintf(stderr, "[libcxlspeckv] " __VA_ARGS__); fputc('\n', stderr); } } while (0)

#define HIP_TRY(expr)                                                              \
    do {                                                                           \
        hipError_t _e = (expr);                                                    \
        if (_e != hipSuccess) {                                                    \
            SPECKV_ERR("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            (void)hipGetLastError();                                               \
            return SPECKV_ERR_DRIVER;                                              \
        }                                                                          \
    } while (0)
#define RC_TRY(expr) do { int _rc = (expr); if (_rc != SPECKV_OK) return _rc; } while (0)

constexpr uint32_t kResSlots = 64;          // flush result words in rotation
constexpr uint32_t kMaxFlights = 16;        // flushes in flight before the oldest is waited for
constexpr uint32_t kUpdCap = 1u << 16;      // mirror-update ring entries

size_t env_mb(const char* name, size_t def_mb)
{
    const char* e = getenv(name);
    if (!e || !*e) return def_mb;
    return static_cast<size_t>(strtoull(e, nullptr, 10));
}

// The C ABI may be called with any HIP device current (SURVEY 8b "Threading"): every entry that touches the
// GPU makes the engine's device current for its own duration and restores the caller's on every exit path.
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int device)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) switched = hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() { if (switched && prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

uint32_t stride_for(int scheme)
{
    switch (scheme) {
    case SPECKV_COMP_INT8: return 2048u;
    case SPECKV_COMP_FP8_E4M3: return 2048u;
    case SPECKV_COMP_INT4_G32: return kInt4RecBytes;      // 1152 B: the 4:1 format (3.56:1 with scales)
    case SPECKV_COMP_MXFP4: return kMx4RecBytes;          // 1088 B per record (3.76:1), but NOT a stride: the pool holds them tile-planar (kernels.hpp, planar_mx4)
    default: return kPageSize;
    }
}

// MXFP4 runs are tile-planar (kernels.hpp: 16 records = 16 nibble rows + 16 code rows = 136 lines): bytes of a run of `recs`
// records, and the table entry of record r of the run at `base`
bool planar_mx4(int scheme) { return scheme == SPECKV_COMP_MXFP4; }
float bits_as_float(uint32_t u) { float f; memcpy(&f, &u, sizeof(f)); return f; }
uint32_t float_bits(float f) { uint32_t u; memcpy(&u, &f, sizeof(u)); return u; }
size_t run_bytes_for(int scheme, uint32_t stride, uint64_t recs)
{
    return planar_mx4(scheme) ? static_cast<size_t>(mx4_run_bytes(recs)) : static_cast<size_t>(recs) * stride;
}
PageEntry entry_at(int scheme, uint32_t stride, uint64_t base, uint64_t r)
{
    if (planar_mx4(scheme)) return PageEntry{base + mx4_nib_off(r), 0u, bits_as_float(mx4_code_delta(r))};
    return PageEntry{base + r * stride, 0u, 1.0f};
}
// granule in which a fragmented pool serves such runs, and the records a piece of `bytes` holds
size_t run_granule_for(int scheme, uint32_t stride) { return planar_mx4(scheme) ? kMx4TileBytes : stride; }
uint64_t run_records_for(int scheme, uint32_t stride, size_t bytes) { return planar_mx4(scheme) ? bytes / kMx4TileBytes * kMx4TileRecs : bytes / stride; }

int no_data_path(const char* what)
{
    static bool warned = false;
    if (!warned) {
        SPECKV_ERR("%s: the \"/dev/null\" device has no data path (page-table emulation only); "
                   "open a HIP device to move or decode KV blocks", what);
        warned = true;
    }
    return SPECKV_ERR_DRIVER;
}

bool is_capturing(hipStream_t s)
{
    if (!s) return false;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

std::vector<int> parse_int_list(const char* env)
{
    std::vector<int> out;
    if (!env) return out;
    std::string s(env);
    size_t i = 0;
    while (i < s.size()) {
        size_t j = s.find(',', i);
        if (j == std::string::npos) j = s.size();
        if (j > i) out.push_back(atoi(s.substr(i, j - i).c_str()));
        i = j + 1;
    }
    return out;
}

// the tuning keys the batch attention's launch decision reads (attend_geometry.hpp takes them as values)
BatchTuning batch_tuning()
{
    const Tuning& t = tuning();
    return BatchTuning{t.attend_tiles_per_split, t.attend_order_as_given, t.attend_fp8_table_regs, t.attend_fp8_striped_table, t.attend_int4_striped_wg};
}

// ... and the single-sequence entries' (qk_scores_fp8, attend_fp8 / _int4 / _mx4)
SeqTuning seq_tuning()
{
    const Tuning& t = tuning();
    return SeqTuning{t.attend_general, t.attend_splits, t.attend_stream, t.attend_fp8_table_regs, t.attend_fp8_striped_table, t.attend_int4_striped_wg, t.attend_fp8_dma};
}

// The region rule of an allocation of the split pool (FP8 keys in one, MXFP4 values in the other): scheme `want`, 8 x 128 fp16 per
// position, num_tokens a multiple of `tokens_multiple`, pos_end inside it, and region `layer` (num_tokens / 2 pages) inside its pages
bool split_region_ok(const Allocation* a, int want, uint32_t layer, uint32_t pos_end, uint32_t tokens_multiple)
{
    if (!a->has_layout || a->scheme != want) return false;
    const Layout& L = a->layout;
    if (L.head_dim != 128 || L.bytes_per_element != 2 || L.num_heads != 8 || L.num_tokens % tokens_multiple || pos_end > L.num_tokens) return false;
    return (static_cast<uint64_t>(layer) + 1u) * (L.num_tokens / 2u) <= a->n_pages && layer < 2ull * L.num_layers;
}

// A batch launch reads its descriptor slot in place: whatever was launched must have passed before the slot is written again.  The
// slot's event is recorded on EVERY way out of the scope that holds the guard (a merge launch that fails behind an
// attention launch that went through used to leave the slot unguarded under a kernel still fetching from it).
struct SlotGuard {
    hipEvent_t ev; hipStream_t st;
    ~SlotGuard() { if (hipEventRecord(ev, st) != hipSuccess) (void)hipGetLastError(); }
};

} // namespace

// A step of a batch whose descriptors are staged per call (the decode and draft entries of engine_attend_kv.cpp and engine_attend_spec.cpp),
// once its members stand: n_splits of a descriptor = the member's tiles until assign_pieces.  tiles / pages are the members of the launch
// decision and may outnumber the sequences (attend_layers_kv: [layer][sequence]); everything else is per sequence.
struct Engine::StagedStep {
    const char* entry;                           // for messages
    std::vector<AttendSeq> seqs;
    std::vector<AttendKvSide> vside;             // the second allocation of a member of the split pool; empty: one allocation per sequence
    std::vector<uint32_t> tiles, pages;
    std::vector<uint32_t> skip;                  // AttendArgs::seq_skip, staged where not empty (a window's skip or rel array)
    std::vector<Allocation*> allocs;             // what speckv_free must wait for
    uint64_t total_tiles = 0;
    bool fp8 = true, mx4 = false;                // the BatchShape whose launch decision the kernel follows
    uint32_t copies = 1;                         // the partials are this many times those of the pieces (2: the wide kernels; the layers of a launch)
    uint64_t grid_rows = 0;                      // the workgroup rows of a grid that is not rows-first, where they are more than the sequences' (0: not judged)
    const void* d_q_f16; uint32_t g; float sm_scale; float* d_out; float* d_lse;
    StagedStep(const char* entry, size_t n_seq, size_t members, bool split, const void* d_q_f16, uint32_t g, float sm_scale, float* d_out, float* d_lse)
        : entry(entry), seqs(n_seq), vside(split ? n_seq : 0u), tiles(members), pages(members), d_q_f16(d_q_f16), g(g), sm_scale(sm_scale), d_out(d_out), d_lse(d_lse) { allocs.reserve(2u * n_seq); }
};

// What every such entry does behind its members: the launch decision of attend_geometry.hpp over the pages walked, the members' pieces, the scratch,
// ONE slot of the pinned descriptor ring read in place by the kernels (descriptors, V sides, dispatch order, skip array: Engine::attend_batch),
// the arguments every launch takes, the waits -- and the launch itself, which is the caller's: launch(args, the V sides on the device,
// the partials of one copy, whether a merge follows, the stream) -> status, where the entry sets what only it knows and names its kernel.
// NULL = the engine's stream and a synchronous call: the query may have been produced on any stream of the caller.
template <class Launch>
int Engine::staged_launch(StagedStep& m, hipStream_t s, Launch launch)
{
    const auto refuse = [&](const char* why) { SPECKV_ERR("%s: %s", m.entry, why); return SPECKV_ERR_INVAL; };
    DeviceScope device_scope(device_);
    if (!s) HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = s ? s : stream_;
    const uint32_t n_seq = static_cast<uint32_t>(m.seqs.size()), members = static_cast<uint32_t>(m.tiles.size());
    const BatchTuning tun = batch_tuning();
    const BatchShape shape{m.fp8, m.mx4, members, 8u, cus(), false, false};
    const BatchForm form = batch_form(shape, tun);
    std::vector<uint32_t> order(members);
    const bool ordered = batch_dispatch_order(form, tun, m.pages.data(), members, order.data());
    const BatchGeometry geo = batch_geometry(kEntryBatch, shape, form, tun, m.tiles.data(), 0, ordered, nullptr);
    if (!geo.fits) return refuse("a member in more than 2048 pieces");
    const uint64_t parts = assign_pieces(geo, 8u, m.seqs.data(), n_seq);
    bool merge = false;
    for (uint32_t i = 0; i < n_seq; ++i) merge = merge || m.seqs[i].n_splits > 1u;
    AttendArgs k{};
    if ((m.copies > 1u && parts * m.copies > 0xFFFFFFFFull) || (!geo.rows_first && m.grid_rows > 65535u))
        return refuse("a grid beyond the launch limits (the workgroup rows of all members, or more than 2^32 partials)");
    if (!attend_scratch(k, merge ? parts * m.copies : 1u, 0, s)) return SPECKV_ERR_NOMEM;
    const size_t desc_bytes = n_seq * sizeof(AttendSeq), side_bytes = m.vside.size() * sizeof(AttendKvSide), order_bytes = ordered ? members * sizeof(uint32_t) : 0u,
                 skip_bytes = m.skip.size() * sizeof(uint32_t);
    int slot = 0;
    void* staged = nullptr;
    RC_TRY(take_seq_slot(desc_bytes + side_bytes + order_bytes + skip_bytes, &slot, &staged));
    uint8_t* h_slot = static_cast<uint8_t*>(staged);
    memcpy(h_slot, m.seqs.data(), desc_bytes);
    if (side_bytes) memcpy(h_slot + desc_bytes, m.vside.data(), side_bytes);
    if (ordered) memcpy(h_slot + desc_bytes + side_bytes, order.data(), order_bytes);
    if (skip_bytes) memcpy(h_slot + desc_bytes + side_bytes + order_bytes, m.skip.data(), skip_bytes);
    uint8_t* d_slot = nullptr;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_slot), staged, 0));
    k.heads = 8u;
    k.g = m.g;
    k.n_splits = m.total_tiles ? geo.max_splits : 0u;
    k.tiles_per_split = geo.tps;
    k.q16 = static_cast<const uint16_t*>(m.d_q_f16);
    k.scale_log2e = m.sm_scale * 1.4426950408889634f;
    k.lin_base = m.seqs[0].lin_base;                                     // (overridden per sequence)
    k.seqs = reinterpret_cast<const AttendSeq*>(d_slot);
    if (ordered) k.order = reinterpret_cast<const uint32_t*>(d_slot + desc_bytes + side_bytes);
    if (skip_bytes) k.seq_skip = reinterpret_cast<const uint32_t*>(d_slot + desc_bytes + side_bytes + order_bytes);
    if (geo.rows_first) k.rows_first = 1u;
    k.direct_out = m.d_out;
    k.direct_lse = m.d_lse;
    k.direct_per_seq = 1u;                                               // members with one piece or none are final, the merge passes them over
    // behind the asynchronous pool writes on every other caller stream the engine knows (a commit on another stream)
    for (auto& w : write_evs_)
        if (w.s != st) HIP_TRY(hipStreamWaitEvent(st, w.ev, 0));
    for (Allocation* a : m.allocs) note_use(a, s);                       // speckv_free waits for this stream
    // The guard event is recorded on every way out from here on: the slot must not be written again under a kernel still reading it.
    SlotGuard slot_guard{seq_ring_.ev[slot], st};
    RC_TRY(launch(k, reinterpret_cast<const AttendKvSide*>(d_slot + desc_bytes), static_cast<uint32_t>(parts), merge, st));
    if (!s) HIP_TRY(hipStreamSynchronize(stream_));
    return SPECKV_OK;
}

} // namespace speckv
