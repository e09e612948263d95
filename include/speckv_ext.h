/*
 * include/speckv_ext.h -- additive entry points of libcxlspeckv.so.
 *
 * The eight functions of include/speckv.h are the drop-in surface.  The
 * reference C ABI stops at the fake pointer returned by speckv_access: it has
 * no write path (flags bit0 exists only in tests/test_dma.c:42), no way to
 * observe the page table (host/include/speckv_allocator.hpp:49-55 is private),
 * no batch form, and it never reaches its own codec
 * (src/fpga_engine/cache_engine.h:42-56) or prefetcher
 * (src/prefetcher/speculative_prefetcher.h:45-57).  The speckv_ext_* functions
 * below expose exactly those pieces, with plain pointers and sizes only, so
 * that (a) parity can be checked on logical ids and on codec bytes, (b) a
 * serving engine can drive the path in batches.  Each one cites the reference
 * interface it stands in for.
 *
 * Pointers named d_* are DEVICE pointers on the compute GPU.  `stream` is a
 * hipStream_t passed as void*: the work is ordered on it and the call returns
 * without waiting.  NULL = the engine's own stream and a SYNCHRONOUS call: it
 * first waits for the device (the caller's buffers may have been produced on
 * any stream) and returns when the result is complete.  A stream handed to the
 * library must stay alive until speckv_finalize or until the library has been
 * called on another stream after it: the engine orders later work behind the
 * stream that last wrote an allocation or last used one of its scratch buffers
 * by recording an event on that stream.
 */
#ifndef SPECKV_EXT_H
#define SPECKV_EXT_H

#include "speckv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SPECKV_PAGE_SIZE   4096u          /* speckv_allocator.cpp:18,58 */
#define SPECKV_BLOCK_ELEMS 2048u          /* fp16 elements per page */

/* ---- quantiser mode (SURVEY.md sect. 0.4) ----------------------------- */
typedef enum {
    SPECKV_QUANT_REF_EXACT = 0,  /* bit-for-bit cache_engine.cpp:186-196,275-284 */
    SPECKV_QUANT_INTENT    = 1,  /* q=clamp(round(x/s),-127,127), y=q*s (cache_engine.cpp:182, kv_compress.v:130) */
} speckv_quant_mode_t;
speckv_status_t speckv_ext_set_quant_mode(speckv_quant_mode_t mode);

/* ---- DMA descriptor: wire format of the reference (speckv_driver.hpp:9-14,
 *      driver/uapi/speckv_ioctl.h:10-15), 24 bytes -------------------------- */
typedef struct {
    uint64_t fpga_addr;   /* pool-side address (HBM of the pool GPU)            */
    uint64_t gpu_addr;    /* compute-GPU address                                */
    uint32_t bytes;
    uint32_t flags;       /* bit0 0=pool->GPU 1=GPU->pool, bit1 compressed, bit2 prefetch */
} speckv_dma_desc_t;
#define SPECKV_DMA_WRITE      0x1u
#define SPECKV_DMA_COMPRESSED 0x2u
#define SPECKV_DMA_PREFETCH   0x4u

/* ---- page table introspection (KvPageHandle, speckv_allocator.hpp:21-26) */
typedef struct {
    uint64_t virt_page_id;   /* (handle<<32)|(i<<12)          speckv_allocator.cpp:24 */
    uint64_t phys_page_id;   /* 0x4000000000+(h<<20)+(i<<12)  speckv_allocator.cpp:25 */
    uint32_t page_size;      /* 4096 */
    uint32_t flags;          /* bit0 L1, bit1 L2, bit2 compressed */
    int32_t  pool_device;    /* HIP device holding the pool copy, -1 in /dev/null mode */
    uint32_t scheme;         /* speckv_comp_scheme_t of the allocation */
    uint32_t rec_bytes;      /* bytes of the stored record (0 = never written) */
    float    scale;          /* per-block scale factor */
    uint64_t pool_addr;      /* device address of the record in the pool */
    uint64_t cache_addr;     /* device address of the decompressed copy, 0 if not resident */
    uint32_t access_count;   /* MemoryPage::access_count, cxl_memory_manager.h:34 */
    uint32_t aux_offset;     /* 0: the record's rec_bytes are contiguous at pool_addr.  MXFP4 (tile-planar pool, 16 records = 16 nibble
                              * rows + 16 code rows = 136 whole cache lines): bytes 0..1023 at pool_addr, bytes 1024..1087 (the E8M0
                              * codes) at pool_addr + aux_offset.  (The field was `reserved`, always 0, until ABI version 6.) */
} speckv_ext_page_info_t;
speckv_status_t speckv_ext_translate(speckv_handle_t handle, uint64_t offset_bytes,
                                     speckv_ext_page_info_t* out);

/* descriptor the engine would submit for a synchronous fetch of that page
 * (speckv_allocator.cpp:115-127) -- logical ids, for parity */
speckv_status_t speckv_ext_fetch_desc(speckv_handle_t handle, uint64_t offset_bytes,
                                      speckv_dma_desc_t* out);

/* ---- layout of the shim allocation (vllm_speckv_backend.py:26-43,87-100) */
speckv_status_t speckv_ext_set_layout(speckv_handle_t handle, uint32_t num_tokens,
                                      uint32_t num_layers, uint32_t num_heads,
                                      uint32_t head_dim, uint32_t bytes_per_element);

/* ---- data path --------------------------------------------------------- */
/* Populate the pool (compress with the allocation's scheme).  offset and len
 * must be multiples of 4096 (len may run to the end of the allocation).
 * Stands in for the DMA write direction the reference only sketches. */
speckv_status_t speckv_ext_write(speckv_handle_t handle, uint64_t offset_bytes,
                                 const void* src, size_t len, int src_on_device);
/* The append path of a decode loop: compress n pages first_page, first_page + page_step, ... from a contiguous device
 * buffer (n * 4096 bytes), ASYNCHRONOUSLY on `stream` (the source must stay valid until the stream gets there).  In
 * the shim layout the pages of one position pair in all (layer, kind) regions are num_tokens/2 pages apart, so one
 * call stores a sequence's new K and V rows of every layer.  Pages that are cached at the time of the call are
 * invalidated first (that case waits for the engine). */
speckv_status_t speckv_ext_write_strided(speckv_handle_t handle, uint64_t first_page, uint64_t page_step,
                                         uint64_t n_pages, const void* d_src, void* stream);
/* A contiguous page range from a device buffer, ASYNCHRONOUSLY on `stream` and without a device-wide wait (speckv_ext_write
 * with src_on_device waits for the whole device first: its source may come from any stream).  offset and len are
 * multiples of 4096.  Ordering: work the engine later does on its own stream for speckv_access / speckv_ext_read /
 * speckv_prefetch is ordered behind the write by the library; reads the caller issues on OTHER streams of its own
 * (speckv_ext_fetch_range, speckv_ext_attend_*) are the caller's to order, as with any stream. */
speckv_status_t speckv_ext_write_async(speckv_handle_t handle, uint64_t offset_bytes, const void* d_src, size_t len,
                                       void* stream);
/* The same for a batch of sequences in ONE launch: allocation handles[i] gets pages first_pages[i] + j * page_step
 * (j < n_pages_each) from d_srcs[i] + j * 4096.  All allocations must use the same compression scheme and the stream
 * must not be NULL.  (A decode step of 256 sequences appends with one call instead of 256 launches.) */
speckv_status_t speckv_ext_write_strided_batch(const speckv_handle_t* handles, const uint64_t* first_pages,
                                               const void* const* d_srcs, uint32_t n_allocations, uint64_t page_step,
                                               uint64_t n_pages_each, void* stream);
/* The commit of a multi-position decode step in ONE launch, rows gathered by the encoder: pair i is a position pair of
 * allocation handles[i] -- pages first_pages[i] + j * page_step, j < 2 * n_layers, page j being layer j / 2, kind j % 2 (K, V)
 * as in the shim layout.  A page's first 2048 bytes are read from d_rows[4 * i + 2 * kind] + layer * layer_stride_bytes (the
 * even position's row), its second 2048 bytes from d_rows[4 * i + 2 * kind + 1] + layer * layer_stride_bytes (the odd one's):
 * no page image is assembled, the rows may lie in any device tensors (a step's k_new / v_new, a held tail row).  The records
 * are those speckv_ext_write_strided_batch stores for the same bytes laid out contiguously.  An allocation may appear in
 * several pairs as long as no two of them share a page.  Asynchronous on `stream`; the rows must stay alive and unchanged
 * until the stream has passed the call.
 *   SPECKV_ERR_INVAL    NULL stream or arrays, a NULL row or one not 16-byte aligned, layer_stride_bytes not a multiple of 16,
 *                       page_step == 0, allocations of different schemes, two pairs of one allocation that share a page
 *   SPECKV_ERR_GENERAL  an unknown handle, pages that leave the allocation
 * n_pairs == 0 or n_layers == 0: SPECKV_OK, nothing is done.  Cached target pages are invalidated first, as above. */
speckv_status_t speckv_ext_write_pairs(const speckv_handle_t* handles, const uint64_t* first_pages,
                                       const void* const* d_rows /* [n_pairs][4]: K even, K odd, V even, V odd */,
                                       uint32_t n_pairs, uint64_t page_step, uint32_t n_layers,
                                       uint64_t layer_stride_bytes, void* stream);
/* speckv_ext_write_pairs read backwards, argument for argument: the rollback of committed positions.  Pair i names pages
 * first_pages[i] + j * page_step, j < 2 * n_layers, of allocation handles[i] (page j: layer j / 2, kind j % 2).  The first 2048
 * decoded bytes of a page -- the even position's row, [heads][128] fp16 -- go to d_rows[4 * i + 2 * kind] + layer *
 * layer_stride_bytes, the second 2048 to d_rows[4 * i + 2 * kind + 1] + layer * layer_stride_bytes.  A NULL row is not wanted:
 * that half of the page is not written (and, where the format keeps the halves apart, not read).  The bits are the
 * corresponding half of what speckv_ext_fetch_range writes for that page as fp16, for every scheme; a page never written gives
 * zeros.  ONE launch decodes every row where its record lies (linear, striped, migrated and sealed allocations alike; a
 * sealed allocation stays sealed).  Asynchronous on `stream`, behind what the caller queued there before (a commit on the
 * same stream) and behind the asynchronous pool writes (speckv_ext_write_async and its kin) handed to other streams before the
 * call, unless `stream` is capturing; the rows must stay alive until the stream has passed the call.
 *   SPECKV_ERR_INVAL    NULL stream or arrays, a row not 16-byte aligned, layer_stride_bytes not a multiple of 16,
 *                       page_step == 0, allocations of different schemes
 *   SPECKV_ERR_GENERAL  an unknown handle, pages that leave the allocation
 * n_pairs == 0 or n_layers == 0: SPECKV_OK, nothing is done. */
speckv_status_t speckv_ext_read_pairs(const speckv_handle_t* handles, const uint64_t* first_pages,
                                      void* const* d_rows /* [n_pairs][4]: K even, K odd, V even, V odd; NULL = not wanted */,
                                      uint32_t n_pairs, uint64_t page_step, uint32_t n_layers,
                                      uint64_t layer_stride_bytes, void* stream);
/* Paged-cache transfers: spans of positions between the pool and the blocks of a caller's paged KV cache (vLLM's layout: one cache
 * tensor per layer, a row addressed by a slot id), ONE launch per call.  Span i is positions [first_tokens[i], first_tokens[i] +
 * n_tokens[i]) of allocation handles[i] in the shim layout: the page of (layer, kind, position) is (2 * layer + kind) * page_step +
 * position / 2, for the layers [layer_begin, layer_begin + n_layers).  Row t of span i lies in slot d_slots[slot_begins[i] + t] --
 * d_slots is an int64 array ON THE DEVICE, the spans' mappings concatenated (slot_begins are host values) -- and the row of slot s is
 * the 2048 bytes ([heads][128] fp16) at d_caches[l] + kind * kind_stride_bytes + s * 2048, d_caches being a HOST array of n_layers
 * device addresses, d_caches[l] the base of layer layer_begin + l (K plane at 0, V plane at kind_stride_bytes).  A slot that is
 * negative (a padding slot) or >= n_slots names no row.  What is staged per call is one descriptor per span and the n_layers
 * addresses: nothing grows with the token count.
 * speckv_ext_read_slots decodes.  A span may begin and end on any position of the stored (paired) part of an allocation; a position
 * outside its span, or one whose slot names no row, is not written (and, where the format keeps the halves of a page apart, not
 * read).  The bits are those speckv_ext_fetch_range writes for the same pages as fp16, for every scheme and both quantiser modes; a
 * page never written gives zeros.  Ordering and placement as speckv_ext_read_pairs: asynchronous on `stream`, behind what the
 * caller queued there before and behind the asynchronous pool writes handed to other streams before the call; linear, striped,
 * migrated and sealed allocations alike, a sealed allocation stays sealed.
 * speckv_ext_write_slots encodes whole pairs: first_tokens[i] and n_tokens[i] are even.  The records are those
 * speckv_ext_write_runs stores for the same rows laid out contiguously; a slot that names no row is read as a row of zeros, and
 * nothing outside the caches is ever read.  Host side as speckv_ext_write_pairs: a sealed destination is unpacked, cached target
 * pages are invalidated first.  The caches and d_slots must stay alive and unchanged until the stream has passed the call.
 *   SPECKV_ERR_INVAL    NULL stream or arrays, a NULL cache pointer or one not 16-byte aligned, kind_stride_bytes not a multiple of
 *                       16, page_step == 0, allocations of different schemes, a capturing stream; write: an odd first_tokens[i] or
 *                       n_tokens[i], two spans of one allocation that share a page
 *   SPECKV_ERR_GENERAL  an unknown handle, a span that leaves its (layer, kind) region (first + n > 2 * page_step) or the allocation
 * n_spans == 0, n_layers == 0 or every n_tokens[i] == 0: SPECKV_OK, nothing is done.  Every refusal launches nothing.  The pages
 * are counted in total_decompressions (and dma_submitted / dma_completed) or total_compressions like those of the pair entries. */
speckv_status_t speckv_ext_read_slots(const speckv_handle_t* handles, const uint64_t* first_tokens, const uint64_t* n_tokens,
                                      const uint64_t* slot_begins, uint32_t n_spans,
                                      const int64_t* d_slots /* device */, uint64_t n_slots,
                                      void* const* d_caches /* host array of n_layers device pointers */,
                                      uint32_t layer_begin, uint32_t n_layers, uint64_t kind_stride_bytes,
                                      uint64_t page_step, void* stream);
speckv_status_t speckv_ext_write_slots(const speckv_handle_t* handles, const uint64_t* first_tokens, const uint64_t* n_tokens,
                                       const uint64_t* slot_begins, uint32_t n_spans,
                                       const int64_t* d_slots /* device */, uint64_t n_slots,
                                       const void* const* d_caches /* host array of n_layers device pointers */,
                                       uint32_t layer_begin, uint32_t n_layers, uint64_t kind_stride_bytes,
                                       uint64_t page_step, void* stream);
/* The same two calls for caches that hold bf16 and for positions held outside pool and caches.  With elem = SPECKV_SLOT_ELEM_FP16
 * and both held arrays NULL each _ex entry IS the entry above: the same refusals, the same launch, the same bits.
 * elem says what the 2048-byte rows of the caches hold.  The pool does not change with it -- a record means the same whichever
 * cache type it passed through -- so a bf16 row is converted as it is read or written, by exactly these two rules:
 *   bf16 row -> pool   each element becomes fp16 by ONE round-to-nearest-even of its exact value: overflow gives +-inf, a NaN stays a
 *                      NaN, fp16 subnormals are kept and anything smaller rounds to +-0.  That fp16 value is what every scheme
 *                      encodes: the record is the one speckv_ext_write_runs stores for row.to(float16).
 *   pool -> bf16 row   the decoded fp16 value -- the bits speckv_ext_fetch_range writes -- is rounded to bf16 by ONE
 *                      round-to-nearest-even of its exact value (never the decoder's fp32 intermediate rounded straight to bf16:
 *                      two routes out of one record do not disagree).
 * Of a NaN only the position is specified, not the payload.
 * A held row is one position of a span, per kind, that lives in neither: [heads][128] fp16 WHATEVER elem says, the row of layer
 * layer_begin + l at pointer + l * held_layer_stride_bytes.  d_held_in / d_held_out are HOST arrays [n_spans][2] (K, V) of device
 * pointers, or NULL; an entry pair is both NULL (no held row for that span) or both set.
 *   read_ex,  d_held_in[2i + kind] set: the span's last position first + n - 1 is even and n >= 1; its row is copied (converted if
 *             elem is bf16) from the held row into its slot, and its page -- never written -- is not read.  Every other position
 *             goes as in speckv_ext_read_slots.
 *   write_ex, d_held_in[2i + kind] set: first_tokens[i], the first position that comes from the caches, is odd, and position
 *             first - 1 comes from the held row: pair (first - 1) / 2 is encoded from one held fp16 row and one cache row.
 *             n_tokens[i] counts cache rows only, row t in d_slots[slot_begins[i] + t].
 *   write_ex, d_held_out[2i + kind] set: first + n is odd; the last position is not encoded but written to the held-out row as
 *             fp16, zeros where its slot names no row.  A span may have both (first = 5, n = 4 encodes pairs 2 and 3 and holds
 *             position 8; first even, n = 1 only moves a row into the held-out block).
 * Still one launch, one descriptor per span; spans of one allocation that share a page are refused, the pair through a held-in row
 * counting as a page of its span; sealed destinations are unpacked, cached target pages invalidated, the pages moved counted as
 * above.  The held rows must stay alive (held-in ones unchanged) until the stream has passed the call.
 *   SPECKV_ERR_INVAL    everything the entries above refuse with it, and: an unknown elem, reserved != 0, a held pointer not 16-byte
 *                       aligned, held_layer_stride_bytes not a multiple of 16, only one of a span's K / V pointers given, a held row
 *                       for an empty span; read: d_held_out not NULL, held-in on a span whose last position is odd; write: an odd
 *                       first without held-in or held-in with an even first, an odd first + n without held-out or held-out with an
 *                       even first + n
 * Every refusal launches nothing and leaves the held-out rows untouched.  Not built: capture into a HIP graph, rows of any other
 * size than 2048 bytes.
 * The _kmul entries below are the _ex entries with a per-channel factor on K (a K pre-scale: K / scale in the pool, q * scale against
 * it).  d_k_mul is a DEVICE pointer to fp16 [heads][128] factor rows (2048 bytes), the row of layer layer_begin + l at d_k_mul +
 * l * k_mul_layer_stride_bytes -- relative to layer_begin like d_caches and the held rows.  With d_k_mul == NULL each _kmul entry IS
 * the _ex entry: the same refusals, the same kernel instances, the same bits and statistics.  Otherwise, the one rule: every K
 * element that crosses the boundary between a cache row and the pool side is multiplied by the factor of its (layer, head,
 * channel).  Records and held rows are the pool side (a held row is a tail, and tails hold pre-scaled K).  The product is taken
 * exactly in fp32 (fp16 x fp16 and bf16 x fp16 are exact there) and THAT is rounded once, to nearest even, to the destination's
 * element type -- well defined for any finite factor, not only powers of two.  V is never touched.  Element p of a page block takes
 * factor element p & 1023: the two position rows of a page share the factor row.
 *   write, cache row -> record   the encoder sees fp16_rne(float(x) * float(m)) of the fp16 or bf16 cache element x (for bf16 ONE
 *                                rounding, not bf16 -> fp16 -> scaled); the record is the one speckv_ext_write_runs stores for those
 *                                rows.  A slot that names no row reads zeros as above.
 *   write, held-in row           pool-side already: encoded as it is, not multiplied.
 *   write, held-out row          K is multiplied and rounded to fp16; V is copied or converted as above.
 *   read, record -> cache row    the decoded fp16 value -- the bits speckv_ext_fetch_range writes, never the decoder's fp32
 *                                intermediate -- is multiplied by m and rounded once to fp16 or bf16.
 *   read, held-in row -> slot    K is multiplied and rounded to the caches' element type; V goes as above.
 * With fp16 caches the bits are those of a half-precision multiply of the row (IEEE: the exact product rounded once).
 *   SPECKV_ERR_INVAL    everything the _ex entries refuse with it, and: d_k_mul not 16-byte aligned, k_mul_layer_stride_bytes not
 *                       a multiple of 16 (with d_k_mul set)
 * Every refusal launches nothing and leaves the held-out rows untouched.  The factor rows must stay alive and unchanged until the
 * stream has passed the call. */
#define SPECKV_SLOT_ELEM_FP16 0u
#define SPECKV_SLOT_ELEM_BF16 1u
typedef struct {
    uint32_t elem;                      /* SPECKV_SLOT_ELEM_*: element type of the caches' rows (2048 B either way) */
    uint32_t reserved;                  /* 0 */
    const void* const* d_held_in;       /* NULL, or host array [n_spans][2] of device pointers (each NULL or an fp16 row block) */
    void* const* d_held_out;            /* write only: the same shape, where the launch puts the new odd last position as fp16 */
    uint64_t held_layer_stride_bytes;   /* a multiple of 16 */
} speckv_ext_slot_rows_t;
speckv_status_t speckv_ext_read_slots_ex(const speckv_handle_t* handles, const uint64_t* first_tokens, const uint64_t* n_tokens,
                                         const uint64_t* slot_begins, uint32_t n_spans,
                                         const int64_t* d_slots /* device */, uint64_t n_slots,
                                         void* const* d_caches /* host array of n_layers device pointers */,
                                         uint32_t layer_begin, uint32_t n_layers, uint64_t kind_stride_bytes,
                                         uint64_t page_step, const speckv_ext_slot_rows_t* rows, void* stream);
speckv_status_t speckv_ext_write_slots_ex(const speckv_handle_t* handles, const uint64_t* first_tokens, const uint64_t* n_tokens,
                                          const uint64_t* slot_begins, uint32_t n_spans,
                                          const int64_t* d_slots /* device */, uint64_t n_slots,
                                          const void* const* d_caches /* host array of n_layers device pointers */,
                                          uint32_t layer_begin, uint32_t n_layers, uint64_t kind_stride_bytes,
                                          uint64_t page_step, const speckv_ext_slot_rows_t* rows, void* stream);
speckv_status_t speckv_ext_read_slots_kmul(const speckv_handle_t* handles, const uint64_t* first_tokens, const uint64_t* n_tokens,
                                           const uint64_t* slot_begins, uint32_t n_spans,
                                           const int64_t* d_slots /* device */, uint64_t n_slots,
                                           void* const* d_caches /* host array of n_layers device pointers */,
                                           uint32_t layer_begin, uint32_t n_layers, uint64_t kind_stride_bytes,
                                           uint64_t page_step, const speckv_ext_slot_rows_t* rows,
                                           const void* d_k_mul /* device, fp16 [heads][128] per layer, or NULL */,
                                           uint64_t k_mul_layer_stride_bytes, void* stream);
speckv_status_t speckv_ext_write_slots_kmul(const speckv_handle_t* handles, const uint64_t* first_tokens, const uint64_t* n_tokens,
                                            const uint64_t* slot_begins, uint32_t n_spans,
                                            const int64_t* d_slots /* device */, uint64_t n_slots,
                                            const void* const* d_caches /* host array of n_layers device pointers */,
                                            uint32_t layer_begin, uint32_t n_layers, uint64_t kind_stride_bytes,
                                            uint64_t page_step, const speckv_ext_slot_rows_t* rows,
                                            const void* d_k_mul /* device, fp16 [heads][128] per layer, or NULL */,
                                            uint64_t k_mul_layer_stride_bytes, void* stream);
/* The _ex entries for the split pool ("K8V4"): span i is positions of TWO allocations, k_handles[i] (SPECKV_COMP_FP8_E4M3) holding its
 * K rows and v_handles[i] (SPECKV_COMP_MXFP4) holding its V rows, still ONE launch per call.  Additive: SPECKV_EXT_ABI_VERSION stays
 * as it is.  The contract is that of speckv_ext_read_slots_ex / speckv_ext_write_slots_ex -- spans, d_slots, d_caches (K plane at 0, V
 * plane at kind_stride_bytes), elem, held rows, ordering, placement, sealed destinations, statistics (2 * n_layers pages per position
 * pair) -- except:
 *   addressing  each allocation holds ONE kind, one region per layer: the page of (layer, position) is layer * page_step +
 *               position / 2 in the K allocation and in the V allocation alike, for the layers [layer_begin, layer_begin + n_layers).
 *   read        the K plane of a slot gets the bits speckv_ext_fetch_range writes as fp16 for that page of the K allocation, the V
 *               plane those of the V allocation; bf16 caches get each value rounded once, as above.  A page never written gives zeros.
 *   write       the records in each allocation are those speckv_ext_write_runs stores there for the same rows laid out contiguously
 *               (from bf16 caches: for row.to(float16)).  Held rows are [heads][128] fp16 per kind as above; both allocations of a
 *               span are unpacked if sealed and their cached pages invalidated.
 *   rows        may be NULL: fp16 caches and no held rows.
 *   SPECKV_ERR_INVAL    everything the _ex entries refuse with it (different schemes aside), and: k_handles[i] not FP8_E4M3 or
 *                       v_handles[i] not MXFP4, k_handles[i] == v_handles[i], a NULL handle array; write: two spans that share a
 *                       page in either allocation
 *   SPECKV_ERR_GENERAL  an unknown handle, a span that leaves its region (first + n > 2 * page_step), pages that leave either allocation
 * Every refusal launches nothing and leaves the held-out rows untouched.  Not built: a K factor (_kmul) for the split pool, capture
 * into a HIP graph, rows of any other size than 2048 bytes. */
speckv_status_t speckv_ext_read_slots_kv(const speckv_handle_t* k_handles, const speckv_handle_t* v_handles,
                                         const uint64_t* first_tokens, const uint64_t* n_tokens,
                                         const uint64_t* slot_begins, uint32_t n_spans,
                                         const int64_t* d_slots /* device */, uint64_t n_slots,
                                         void* const* d_caches /* host array of n_layers device pointers */,
                                         uint32_t layer_begin, uint32_t n_layers, uint64_t kind_stride_bytes,
                                         uint64_t page_step, const speckv_ext_slot_rows_t* rows /* NULL = fp16, no held rows */,
                                         void* stream);
speckv_status_t speckv_ext_write_slots_kv(const speckv_handle_t* k_handles, const speckv_handle_t* v_handles,
                                          const uint64_t* first_tokens, const uint64_t* n_tokens,
                                          const uint64_t* slot_begins, uint32_t n_spans,
                                          const int64_t* d_slots /* device */, uint64_t n_slots,
                                          const void* const* d_caches /* host array of n_layers device pointers */,
                                          uint32_t layer_begin, uint32_t n_layers, uint64_t kind_stride_bytes,
                                          uint64_t page_step, const speckv_ext_slot_rows_t* rows /* NULL = fp16, no held rows */,
                                          void* stream);
/* Fork: the STORED RECORDS of page runs copied from one allocation to another, nothing decoded.  Pair i copies pages
 * [run_firsts[r], run_firsts[r] + n_pages[i]) for every run r < n_runs from allocation src[i] to the same page numbers of
 * allocation dst[i] (in the shim layout the runs are the 2 * num_layers (layer, kind) regions and n_pages[i] = positions / 2: a
 * request started from positions another request holds).  ONE launch on `stream` for the whole call.  Afterwards every reader --
 * speckv_ext_fetch_range, speckv_ext_read_pairs, every speckv_ext_attend_* form -- gives the same bits for a copied page of dst[i]
 * as for the page of src[i], and speckv_ext_translate reports the same rec_bytes and the same scale (MXFP4 has no block scale: its
 * aux_offset belongs to the record's slot and stays the destination's own).  A source page never written leaves the destination
 * page never written: rec_bytes 0, decoding to zeros.  All schemes.  Source and destination may each be linear, striped over pools,
 * migrated page by page or sealed; a sealed source stays sealed, a sealed destination is unpacked first, as by any write.
 * Aliasing, for the pairs with n_pages[i] > 0: one source may feed several destinations; an allocation is the destination of ONE
 * pair at most (every pair writes the same page numbers, so two pairs into one allocation would share a destination page), and an
 * allocation that is a destination is not a source in the same call (its pages would be read while they are written);
 * src[i] == dst[i] is refused for every pair.
 * Asynchronous on `stream`.  The sources are read behind what the caller queued there before (a commit on the same stream) and
 * behind the asynchronous pool writes handed to other streams before the call, unless `stream` is capturing; the destinations are
 * written like speckv_ext_write_pairs writes (cached destination pages are invalidated first).
 *   SPECKV_ERR_INVAL    NULL stream or arrays, allocations of different schemes, src[i] == dst[i], a destination named by two pairs
 *                       or also named as a source, runs that overlap -- nothing is launched
 *   SPECKV_ERR_GENERAL  an unknown handle, pages that leave either allocation
 * n_pairs == 0, n_runs == 0 or every n_pages[i] == 0: SPECKV_OK, nothing is done.  Counted in
 * speckv_ext_stats_t.copied_pages (and dma_submitted / dma_completed). */
speckv_status_t speckv_ext_copy_runs(const speckv_handle_t* src, const speckv_handle_t* dst,
                                     const uint64_t* n_pages /* [n_pairs] pages per run of pair i */, uint32_t n_pairs,
                                     const uint64_t* run_firsts /* [n_runs] first page of each run, the same in src and dst */,
                                     uint32_t n_runs, void* stream);
/* speckv_ext_read_pairs and speckv_ext_copy_runs for the split pool ("K8V4"): pair i names TWO allocations per role, an FP8_E4M3 one that
 * holds a request's K rows and an MXFP4 one that holds its V rows, each laid out as ONE region per layer.  Both entries do for both
 * allocations of every pair what their parents do for one, with ONE staged descriptor array and ONE launch per call (the parents refuse
 * a call that mixes schemes, so a split request would cost two calls and two launches).  Additive: SPECKV_EXT_ABI_VERSION stays as it
 * is.
 * speckv_ext_read_pairs_kv: the page of layer l < n_layers of pair i is first_pages[i] + l * page_step in k_handles[i] and in
 * v_handles[i] alike -- n_layers counts real layers, there is no factor 2 and no kind term.  d_rows[4 * i + 0 .. 3] are K even, K odd,
 * V even, V odd: the first 2048 decoded bytes of the K page of layer l go to d_rows[4 * i] + l * layer_stride_bytes, the second 2048
 * to d_rows[4 * i + 1] + l * layer_stride_bytes, those of the V page to d_rows[4 * i + 2] / d_rows[4 * i + 3] in the same way.  A NULL
 * row is not written (and in the FP8 allocation not read).  The bits are the halves of what speckv_ext_fetch_range writes for the
 * page of the K allocation and of the V allocation as fp16; a page never written gives zeros.  Ordering, placement (linear, striped,
 * migrated, sealed; a sealed allocation stays sealed) and statistics (2 * n_layers pages per pair) as speckv_ext_read_pairs.
 *   SPECKV_ERR_INVAL    what speckv_ext_read_pairs refuses with it (different schemes aside), a NULL handle array, k_handles[i] not
 *                       FP8_E4M3 or v_handles[i] not MXFP4, the two allocations of a pair laid out for different num_tokens
 *   SPECKV_ERR_GENERAL  an unknown handle, pages that leave either allocation
 * speckv_ext_copy_runs_kv: pair i copies pages [run_firsts[r], run_firsts[r] + n_pages[i]), every run r, from k_src[i] to k_dst[i] and
 * from v_src[i] to v_dst[i]; per allocation pair the contract of speckv_ext_copy_runs (records, not values; the FP8 block scales in
 * the destination's scale table; the MXFP4 codes at the destination slot's own offset; a source page never written leaves the
 * destination page never written; sealed destinations unpacked, cached destination pages invalidated).  Aliasing is judged ACROSS both
 * sides: an allocation that is written is named once in k_dst and v_dst together and is not named in k_src or v_src.
 *   SPECKV_ERR_INVAL    what speckv_ext_copy_runs refuses with it (different schemes aside), a NULL handle array, a K handle that is
 *                       not FP8_E4M3 or a V handle that is not MXFP4, source == destination on either side, a destination named twice
 *                       (on one side or on both) or also named as a source, allocations of a pair laid out for different num_tokens
 *   SPECKV_ERR_GENERAL  an unknown handle, pages that leave any of the four allocations
 * Counted in speckv_ext_stats_t.copied_pages: 2 * n_runs * n_pages[i] records per pair.  Every refusal launches nothing. */
speckv_status_t speckv_ext_read_pairs_kv(const speckv_handle_t* k_handles, const speckv_handle_t* v_handles,
                                         const uint64_t* first_pages,
                                         void* const* d_rows /* [n_pairs][4]: K even, K odd, V even, V odd; NULL = not wanted */,
                                         uint32_t n_pairs, uint64_t page_step, uint32_t n_layers,
                                         uint64_t layer_stride_bytes, void* stream);
speckv_status_t speckv_ext_copy_runs_kv(const speckv_handle_t* k_src, const speckv_handle_t* v_src,
                                        const speckv_handle_t* k_dst, const speckv_handle_t* v_dst,
                                        const uint64_t* n_pages /* [n_pairs] pages per run of pair i */, uint32_t n_pairs,
                                        const uint64_t* run_firsts /* [n_runs] first page of each run, the same in all four */,
                                        uint32_t n_runs, void* stream);
/* Several page runs of ONE allocation in one launch: run r = pages [first_pages[r], first_pages[r] + n_pages_each) from
 * d_srcs[r] (n_pages_each * 4096 contiguous bytes).  A prompt's K and V of every layer (2 * num_layers regions of the shim
 * layout) are stored with one call.  The runs must not overlap; the stream must not be NULL. */
speckv_status_t speckv_ext_write_runs(speckv_handle_t handle, const uint64_t* first_pages, const void* const* d_srcs,
                                      uint32_t n_runs, uint64_t n_pages_each, void* stream);
/* Fetch + decompress straight into a caller buffer, bypassing the tiers. */
speckv_status_t speckv_ext_read(speckv_handle_t handle, uint64_t offset_bytes,
                                void* dst, size_t len, int dst_on_device);
/* The bulk hot path: fetch + decompress pages [first_page, first_page+n) of a
 * handle into d_dst (n * 2048 elements, fp16 if out_f32==0 else fp32).
 * Asynchronous on `stream`.  One kernel launch. */
speckv_status_t speckv_ext_fetch_range(speckv_handle_t handle, uint64_t first_page,
                                       uint64_t n_pages, void* d_dst, int out_f32,
                                       void* stream);
/* The same with the fetch engine chosen by the caller: 0 = per batch (long runs on remote pools -> copy engines,
 * everything else -> fused kernel; SPECKV_REMOTE_ENGINE=kernel|copy overrides), 1 = fused peer-load + decompress
 * kernel, 2 = copy engines: the range's contiguous record runs (one per pool GPU, because pages are striped) are
 * copied with hipMemcpyPeerAsync on per-peer side streams into local staging and decompressed from there,
 * double-buffered.  Stands in for the reference's DMA path (one descriptor per page through the DMA engine:
 * host/src/speckv_allocator.cpp:115-138, hardware/rtl/dma_engine.v:150-217).  Engine 2 needs the default striped
 * placement (SPECKV_ERR_INVAL after a migration or on a fragmented allocation). */
speckv_status_t speckv_ext_fetch_range_engine(speckv_handle_t handle, uint64_t first_page,
                                              uint64_t n_pages, void* d_dst, int out_f32,
                                              void* stream, int engine);
/* Same for an arbitrary device-resident page list. */
speckv_status_t speckv_ext_fetch_list(speckv_handle_t handle, const uint32_t* d_pages,
                                      uint32_t n, void* d_dst, int out_f32, void* stream);
/* Batched speckv_access: out_ptrs[i] = device address of offsets[i]. */
speckv_status_t speckv_ext_access_batch(speckv_handle_t handle, const uint64_t* offsets,
                                        uint32_t n, void** out_ptrs);

/* ---- speculative prefetch (speculative_prefetcher.cpp:25-82, prefetch_core.v:150-241) */
/* Which allocation a request id of speckv_prefetch / speckv_ext_prefetch_batch addresses: request `req_id` is
 * request `local_req` of `handle`'s layout (one allocation per sequence: local_req 0).  handle 0 removes the binding.
 * Unbound request ids index into the most recently laid-out (else most recently allocated) allocation, as in the
 * reference's single-allocation shim (vllm_speckv_backend.py:95-100); requests that address nothing are counted in
 * speckv_ext_stats_t.prefetch_dropped. */
speckv_status_t speckv_ext_bind_request(uint32_t req_id, speckv_handle_t handle, uint32_t local_req);
/* Batched speckv_prefetch: host arrays of n requests (see speckv_ext_bind_request). */
speckv_status_t speckv_ext_prefetch_batch(uint32_t n, const uint32_t* req_ids,
                                          const uint16_t* layers, const uint32_t* cur_pos,
                                          const uint32_t* depth_k);
/* Drain queued prefetch requests now: candidates, residency filter, dedupe, ring-slot assignment and the fetch all
 * run on the device; the call only submits (no host round trip).  n_issued may be NULL; when given, the call waits
 * for the (small) assignment kernel and returns the number of pages being fetched into L2. */
speckv_status_t speckv_ext_prefetch_flush(uint32_t* n_issued);
/* The raw lookup kernel on device buffers: for request r, candidate pages of
 * positions cur_pos+1..cur_pos+depth_k (K then V), residency-filtered with the
 * handle's device flag mirror, compacted in request order into d_out_pages.
 * *d_out_count receives the total.  Deterministic. */
speckv_status_t speckv_ext_prefetch_lookup(speckv_handle_t handle, uint32_t n,
                                           const uint32_t* d_req_ids, const uint32_t* d_layers,
                                           const uint32_t* d_cur_pos, const uint32_t* d_depth_k,
                                           uint32_t* d_out_pages, uint32_t cap,
                                           uint32_t* d_out_count, void* stream);
/* Legacy address list of the reference's CPU prefetcher
 * (speculative_prefetcher.cpp:48,153-160): (0<<32)|(layer<<16)|(i+1). */
speckv_status_t speckv_ext_prefetch_legacy_addrs(uint32_t layer, uint32_t depth_k,
                                                 uint64_t* out_addrs, uint32_t* out_n);

/* Token predictor (LSTMPredictor, src/prefetcher/lstm_predictor.cpp:40-188).
 * The reference draws its weights from rand(); here the caller supplies them:
 * embedding [vocab][64], out_weights [vocab][128] (fp32, host or device).  Once loaded,
 * speckv_prefetch keeps the last 16 tokens per request, each flush predicts the next
 * tokens of the requests whose history changed (top-depth, depth <= 8) -- on a stream of the
 * engine's own, without holding the flush up: the pages a flush fetches are addressed by
 * position, the tokens only feed the hit statistics -- and
 * speckv_ext_verify(req, actual, NULL, 0) checks against that prediction (waiting for it
 * if it is still on its way).
 * speckv_ext_predict_batch is the raw operator: n histories of 16 int32 tokens
 * (device) -> top-k tokens / confidences (device, k <= 8). */
speckv_status_t speckv_ext_predictor_load(const float* embedding, const float* out_weights,
                                          uint32_t vocab, int on_device);
/* A REAL LSTM cell for the same predictor.  The reference's cell is degenerate (gates fixed at 0.5, recurrent weights never
 * read: lstm_predictor.cpp:117-146), which speckv_ext_predictor_load reproduces for parity; its semantics as a model are
 * therefore defined here: the standard LSTM with PyTorch's nn.LSTM conventions --
 *     gates = w_ih[l] x + b_ih[l] + w_hh[l] h + b_hh[l]   (rows [i | f | g | o], 4 x 128 each)
 *     c' = sigmoid(f) c + sigmoid(i) tanh(g),   h' = sigmoid(o) tanh(c'),   h_0 = c_0 = 0
 * n_layers <= 4 stacked layers (layer l > 0 is fed layer l-1's h of the same step), input = the 64-wide embedding of each of
 * the last 16 tokens, output layer logits = out_weights [vocab][128] . h_top + out_bias (may be NULL), softmax, top-k.
 * w_ih[0] is [512][64], w_ih[l > 0] and every w_hh[l] [512][128], biases [512]; fp32, host or device.  Replaces any earlier
 * predictor; speckv_ext_predictor_load switches back to the reference's cell. */
speckv_status_t speckv_ext_predictor_load_lstm(const float* embedding, uint32_t vocab, uint32_t n_layers,
                                               const float* const* w_ih, const float* const* w_hh,
                                               const float* const* b_ih, const float* const* b_hh,
                                               const float* out_weights, const float* out_bias, int on_device);
speckv_status_t speckv_ext_predict_batch(uint32_t n, const int32_t* d_histories, uint32_t k,
                                         int32_t* d_tokens, float* d_conf, void* stream);

/* Verification + adaptive depth (speculative_prefetcher.cpp:84-137).  predicted == NULL
 * verifies against the engine's own prediction for req_id (needs a loaded predictor). */
speckv_status_t speckv_ext_verify(uint32_t req_id, int32_t actual_token,
                                  const int32_t* predicted, uint32_t n_predicted,
                                  uint32_t* was_hit, uint32_t* new_depth);
/* Batched token-compare kernel: hit[r] = actual[r] in predicted[r*k .. r*k+k). */
speckv_status_t speckv_ext_verify_batch(uint32_t n, uint32_t k, const int32_t* d_actual,
                                        const int32_t* d_predicted, uint8_t* d_hit,
                                        uint32_t* d_hit_count, void* stream);
speckv_status_t speckv_ext_get_prefetch_depth(uint32_t* depth_k);

/* ---- completion queue (SpeckvDriver::poll_complete, speckv_driver.cpp:65-72;
 *      kernel side speckv_kernel_module.c:194-215): descriptors completed
 *      since the previous poll. */
speckv_status_t speckv_ext_poll_complete(uint32_t* done);
speckv_status_t speckv_ext_sync(void);

/* ---- raw codec operators on caller-owned device buffers -------------------
 * FPGACacheEngine::compress / ::decompress (cache_engine.cpp:40-116) applied
 * per 2048-element KV block.  Work without speckv_init (need a HIP device). */
speckv_status_t speckv_ext_codec_compress(const void* d_src_f16, uint64_t n_blocks,
                                          void* d_recs, uint64_t rec_stride,
                                          uint32_t* d_rec_bytes, float* d_scales,
                                          int scheme, int quant_mode, void* stream);
/* quant_mode of speckv_ext_codec_decompress may carry this flag: the records are known to be short (structured data, mean
 * record well under 512 bytes).  The launch then takes a decoder instantiation with a fast path for constant runs on
 * 8-element boundaries; the output is bit for bit the same with or without it.  (The engine sets it by itself for
 * allocations sealed by speckv_ext_compact whose packed records average under 512 bytes.) */
#define SPECKV_CODEC_HINT_STRUCTURED 0x100
speckv_status_t speckv_ext_codec_decompress(const void* d_recs, uint64_t rec_stride,
                                            const uint32_t* d_rec_bytes, const float* d_scales,
                                            uint64_t n_blocks, void* d_dst, int out_f32,
                                            int scheme, int quant_mode, void* stream);

/* The same two operators with the reference's own call shape -- a tensor of ANY length (cache_engine.cpp:40-116: n = 11
 * in the survey's known-answer vector, the RTL tile of 1024 x 128 = 131 072 elements): ONE scale over the n elements, ONE
 * int8 delta chain and ONE run-length stream; runs and their 255-element splits cross the 2048-element tiles the work is
 * cut into on the device.
 *   d_src        n_elems values, fp32 (src_f32 != 0: the reference's std::vector<float>) or fp16
 *   d_rle        the stream [value u8][count u8]...; 16-byte aligned, room for 2 * n_elems bytes rounded up to 16
 *   d_rle_bytes  (device) compressed_size;   d_scale (device) scale_factor
 *   d_workspace  256-byte aligned device scratch of speckv_ext_codec_tensor_workspace_bytes(n_elems) /
 *                speckv_ext_codec_tensor_decode_workspace_bytes(rle_bytes) bytes
 * Decompress: dst gets min(sum of counts, dst_cap_elems) elements (fp32 or fp16; 16-byte aligned), *d_n_out (device,
 * optional) that number; an odd trailing byte is dropped and a zero count emits nothing, as in the reference.
 * The decoder takes a stream at any 2-BYTE aligned address (a pair is never split; an odd d_rle is SPECKV_ERR_INVAL): the
 * 16-byte alignment above is what compress needs for the stream it writes, and what lets the decoder load 8 pairs at a time --
 * off it the stream is read pair by pair, slower, with the same result.
 * Pass the tensor's element count as dst_cap_elems when it is known: the library picks its decoder from rle_bytes / 2 pairs
 * against dst_cap_elems (a stream of one pair per element is decoded in one pass over the pairs, one that compresses tile by
 * tile of the output); a capacity far above the real count only costs speed, never correctness.
 * Asynchronous on `stream`; no engine needed. */
size_t speckv_ext_codec_tensor_workspace_bytes(uint64_t n_elems);
size_t speckv_ext_codec_tensor_decode_workspace_bytes(uint64_t rle_bytes);
speckv_status_t speckv_ext_codec_compress_tensor(const void* d_src, uint64_t n_elems, int src_f32, void* d_rle,
                                                 uint64_t* d_rle_bytes, float* d_scale, void* d_workspace,
                                                 size_t workspace_bytes, int quant_mode, void* stream);
speckv_status_t speckv_ext_codec_decompress_tensor(const void* d_rle, uint64_t rle_bytes, float scale, void* d_dst,
                                                   uint64_t dst_cap_elems, int out_f32, uint64_t* d_n_out,
                                                   void* d_workspace, size_t workspace_bytes, int quant_mode, void* stream);

/* The same codec over MANY tensors per launch (round 6).  The reference calls FPGACacheEngine::compress(data, n) once per KV tile
 * (cache_engine.cpp:40-82; the RTL's tile is 1024 x 128 = 131 072 elements, hardware/rtl/kv_compress.v:5-11): at that size one
 * tensor is 64 tiles of work and the single-tensor entry point above is all fixed cost (two launches, a look-back chain that has
 * barely started when it ends).  Here one launch takes thousands of tensors: every tensor its own scale, its own delta chain, its
 * own run-length stream; a tensor's workgroups (16 tiles each) find its max|x| by a rendezvous among themselves and hand their
 * chains on by look-back over the tensor's own status words; a wave takes max|x| from its own tile (fp16 tiles stay in registers for
 * the encode, fp32 tiles are read again out of the L2 / Infinity Cache).  Streams and scales are bit-identical to the single-tensor entry point's and to the reference's, per tensor.
 *   d_tensors  DEVICE array of n_tensors descriptors
 *   max_elems  the host's upper bound on the tensors' lengths (sizes the grid and the workspace; a tensor may be shorter, or empty)
 *   compress:   data = the source (fp16, or fp32 with src_f32), n = its elements, rle = where the stream goes (16-byte aligned),
 *               rle_cap >= 2 n rounded up to 16 (not checked); d_rle_bytes[i] / d_scales[i] receive the stream length / the scale
 *   decompress: data = the destination (16-byte aligned; fp16, or fp32 with out_f32), n = its room in elements (<= max_elems),
 *               rle = the stream (2 max_elems bytes at most; 2-byte aligned, as above), d_rle_bytes[i] / d_scales[i] as compress left them; d_n_out[i] (may be
 *               NULL) = elements decoded, clipped to the room
 *   d_workspace  256-byte aligned, speckv_ext_codec_tensors_workspace_bytes(n_tensors, max_elems) bytes (cleared by the call)
 * Asynchronous on `stream`; no engine needed. */
typedef struct {
    void*    data;
    uint64_t n;
    void*    rle;
    uint64_t rle_cap;
} speckv_ext_tensor_t;       /* 32 bytes */
size_t speckv_ext_codec_tensors_workspace_bytes(uint32_t n_tensors, uint64_t max_elems);
speckv_status_t speckv_ext_codec_compress_tensors(uint32_t n_tensors, const speckv_ext_tensor_t* d_tensors, uint64_t max_elems,
                                                  int src_f32, uint64_t* d_rle_bytes, float* d_scales, void* d_workspace,
                                                  size_t workspace_bytes, int quant_mode, void* stream);
speckv_status_t speckv_ext_codec_decompress_tensors(uint32_t n_tensors, const speckv_ext_tensor_t* d_tensors, uint64_t max_elems,
                                                    const uint64_t* d_rle_bytes, const float* d_scales, int out_f32,
                                                    uint64_t* d_n_out, void* d_workspace, size_t workspace_bytes,
                                                    int quant_mode, void* stream);

/* ---- 4:1 / 2:1 formats + fused dequant-matvec (BASELINE config 5; SURVEY 8a row
 *      A22: no reference counterpart, parity is against oracle/ only) -----------
 * SPECKV_COMP_INT4_G32: record 1152 B = 64 fp16 group scales + 2048 nibbles.
 * SPECKV_COMP_FP8_E4M3: record 2048 B of OCP e4m3fn + one f32 scale per block.
 * SPECKV_COMP_MXFP4:    record 1088 B = 2048 E2M1 nibbles + 64 E8M0 block scales (OCP MX v1.0; speckv_ext_attend_mx4).
 * speckv_ext_qk_scores_fp8: attention scores q.K^T for positions
 * [pos_begin, pos_end) (both even) of `layer`, computed on the matrix cores
 * directly from the FP8 records of the K region (request 0 of the shim layout;
 * needs speckv_ext_set_layout with num_heads*head_dim == 1024, head_dim 128).
 *   d_q_f16 : [num_heads][g][128] fp16 query rows (g <= 16 rows per kv head, GQA)
 *   d_out   : [num_heads][g][pos_end-pos_begin] fp32
 * The query is quantised per row to e4m3 (scale max|q|/448) on the device. */
speckv_status_t speckv_ext_qk_scores_fp8(speckv_handle_t handle, uint32_t layer,
                                         const void* d_q_f16, uint32_t g,
                                         uint32_t pos_begin, uint32_t pos_end,
                                         float* d_out, void* stream);
/* Several layers of the sequence in one launch: d_q_f16 [n_layers][num_heads][g][128],
 * d_out [n_layers][num_heads][g][pos_end-pos_begin]. */
speckv_status_t speckv_ext_qk_scores_fp8_layers(speckv_handle_t handle, uint32_t layer_begin,
                                                uint32_t n_layers, const void* d_q_f16, uint32_t g,
                                                uint32_t pos_begin, uint32_t pos_end,
                                                float* d_out, void* stream);

/* speckv_ext_attend_fp8: the whole decode attention of layers [layer_begin, layer_begin+n_layers)
 * over positions [pos_begin, pos_end) (both even), computed from the FP8 K and V records
 * without materialising fp16 KV:  out = softmax(q.K^T * sm_scale) . V  per kv head.
 *   d_q_f16 : [n_layers][num_heads][g][128] fp16      d_out : [n_layers][num_heads][g][128] fp32
 *   d_lse   : optional [n_layers][num_heads][g] fp32 log-sum-exp of the scaled scores (NULL to skip)
 * Scores on v_mfma_f32_16x16x32_fp8_fp8, weights in f16 against V widened to f16 (exact) on
 * v_mfma_f32_16x16x32_f16, fp32 accumulation; the position range is split across the chip and
 * merged by a second kernel.  Pages never written count as zeros.  Same layout requirement as
 * speckv_ext_qk_scores_fp8.  (second half; oracle: orc_attend_fp8.) */
speckv_status_t speckv_ext_attend_fp8(speckv_handle_t handle, uint32_t layer_begin, uint32_t n_layers,
                                      const void* d_q_f16, uint32_t g, uint32_t pos_begin, uint32_t pos_end,
                                      float sm_scale, float* d_out, float* d_lse, void* stream);

/* speckv_ext_attend_fp8_batch: one decode step of a batch -- the fused FP8 attention of ONE layer for n_seq sequences
 * (one allocation each, request 0 of its shim layout) over positions [0, pos_end[i]) in one launch pair.
 *   handles, pos_end : host arrays of n_seq      d_q_f16 : [n_seq][num_heads][g][128] fp16 (device)
 *   d_out : [n_seq][num_heads][g][128] fp32      d_lse : optional [n_seq][num_heads][g]
 * Every allocation must hold FP8 records with a layout whose num_tokens is a multiple of 32 (SPECKV_ERR_INVAL otherwise).
 * Any placement is served: records in one run or striped regularly over the pools take arithmetic addresses; if a member
 * of the batch has lost its regular placement (pages migrated one by one), the whole launch reads its record addresses
 * from the page tables instead (a few percent slower).  Asynchronous on `stream` (the host arrays are copied before the
 * call returns).  The split partials of all attention calls live in one scratch buffer of the engine: a call on another
 * stream than the previous one is ordered behind it by the library (an event at the old stream's tail), so callers may
 * use several streams, but such calls do not overlap on the device. */
speckv_status_t speckv_ext_attend_fp8_batch(uint32_t n_seq, const speckv_handle_t* handles, uint32_t layer,
                                            const void* d_q_f16, uint32_t g, const uint32_t* pos_end, float sm_scale,
                                            float* d_out, float* d_lse, void* stream);

/* speckv_ext_attend_int4: the same attention over SPECKV_COMP_INT4_G32 records (the 4:1 format).  K and V are
 * dequantised exactly as fetch+decompress does (fp16(q4 * group scale)), the query stays fp16, both products run
 * on v_mfma_f32_16x16x32_f16 with fp32 accumulation: the attention over the decompressed fp16 pages, without
 * writing them.  Records in one local run (the default placement of a one-pool engine) or striped regularly over the
 * pools take the arithmetic-address forms of the kernel; an allocation whose pages were migrated one by one takes the
 * same kernel with its record addresses read from the page table one tile ahead; only ranges that do not start on a
 * 32-position tile, or whose last tile would leave the layer, go through the per-wave page-table kernel.
 * (oracle: orc_attend_f16 over decompressed pages.) */
speckv_status_t speckv_ext_attend_int4(speckv_handle_t handle, uint32_t layer_begin, uint32_t n_layers,
                                       const void* d_q_f16, uint32_t g, uint32_t pos_begin, uint32_t pos_end,
                                       float sm_scale, float* d_out, float* d_lse, void* stream);

/* The batch form for INT4_G32 allocations (arguments as speckv_ext_attend_fp8_batch). */
speckv_status_t speckv_ext_attend_int4_batch(uint32_t n_seq, const speckv_handle_t* handles, uint32_t layer,
                                             const void* d_q_f16, uint32_t g, const uint32_t* pos_end, float sm_scale,
                                             float* d_out, float* d_lse, void* stream);

/* speckv_ext_attend_mx4: the same attention over SPECKV_COMP_MXFP4 records -- the 4:1 format gfx950's matrix cores read
 * natively (OCP Microscaling Formats v1.0: FP4 E2M1 elements, one E8M0 power-of-two scale per 32 elements; record = 1024 B of
 * nibbles -- byte i = element i in the low half, element 1024 + i in the high half: the two positions of a page interleaved --
 * then the 64 scale codes, one per 16 bytes: 1088 B per 4 KiB block, 3.76 : 1.  In the POOL the records of a run lie
 * tile-planar: 16 records = their 16 nibble rows followed by their 16 code rows = 136 whole cache lines, so the pool spends
 * 1088 B per page and the attention fetches nothing but record bytes; speckv_ext_translate reports a page's two pieces,
 * speckv_ext_page_info_t::aux_offset.  The raw operators speckv_ext_codec_* keep contiguous records).
 * q.K^T runs on v_mfma_scale_f32_16x16x128_f8f6f4: one instruction contracts the whole head dimension, K nibbles and scale
 * codes go in as they lie in the record, the block scales are applied by the hardware; the query is quantised to MXFP8
 * (e4m3 elements, E8M0 per 32: emax 8, saturating) on the device.  V is widened to f16 WITH its block scale by one
 * v_cvt_scalef32_pk_f16_fp4 per element pair and meets the f16 softmax weights on v_mfma_f32_16x16x32_f16, fp32 accumulation.
 * Any placement is served (one run, regular striping, page-table addresses).  g <= 16 query rows per kv head, taken in groups
 * of 8 (a second set of workgroups for rows 8 .. 15): the 16 columns of a score MFMA are 8 query rows x the 2 positions of a
 * page, so with g = 8 (GQA 8) every column is live, with g = 4 half of them are masked.
 * (oracle: orc_attend_mx4; arguments as speckv_ext_attend_int4.) */
speckv_status_t speckv_ext_attend_mx4(speckv_handle_t handle, uint32_t layer_begin, uint32_t n_layers,
                                      const void* d_q_f16, uint32_t g, uint32_t pos_begin, uint32_t pos_end,
                                      float sm_scale, float* d_out, float* d_lse, void* stream);
/* The batch and planned forms for MXFP4 allocations (arguments as speckv_ext_attend_fp8_batch / _planned). */
speckv_status_t speckv_ext_attend_mx4_batch(uint32_t n_seq, const speckv_handle_t* handles, uint32_t layer,
                                            const void* d_q_f16, uint32_t g, const uint32_t* pos_end, float sm_scale,
                                            float* d_out, float* d_lse, void* stream);
speckv_status_t speckv_ext_attend_mx4_planned(const void* d_plan, uint32_t n_seq, uint32_t layer, const void* d_q_f16,
                                              uint32_t g, uint32_t max_pos_end, float sm_scale, float* d_out,
                                              float* d_lse, void* stream);

/* ---- planned batches: the batch attention of a decode step under a HIP graph -------------------------------------
 * The batch calls above stage their per-sequence descriptors on every call and cannot be captured.  The planned form
 * splits them in two:
 *   speckv_ext_attend_batch_plan   once per decode step, OUTSIDE any capture: looks the n_seq allocations up and writes
 *       one descriptor per sequence -- valid for every layer -- into the caller's device buffer d_plan
 *       (speckv_ext_attend_plan_bytes(n_seq) bytes; the copy is ordered on `stream`), and behind them the order in which
 *       the launches take the sequences: batches whose members differ in length are dispatched by length (a long member
 *       beside a short one on every CU) -- rows of q / out / lse stay in the caller's order.  A buffer of n_seq x 64 bytes
 *       (what the size was before) still works, in the caller's order.
 *   speckv_ext_attend_{fp8,int4}_planned   one layer of the batch: kernel launches only (no look-ups, no staging,
 *       nothing allocated once the scratch is warm), so the per-layer calls of a step can be captured once and replayed
 *       for as long as every pos_end stays <= max_pos_end: grid and scratch are functions of (n_seq, max_pos_end) and of
 *       what the FIRST plan of that shape written into that buffer saw (a batch whose members differ much in length gets
 *       room for pieces per member and a merge launch; every later plan of the shape in the buffer keeps that room, so the
 *       captured launches stay valid, however many other shapes are planned meanwhile -- the room of a shape is dropped only
 *       once its buffer is no longer one of the engine's plan buffers: more than 64 buffers in use at once drop them all);
 *       the lengths and piece lengths themselves are read from the plan on the device.
 *       Capture AFTER the first plan of a shape, as before.
 * Arguments as for the batch calls; max_pos_end (even) must be the value given to the plan.  `stream` must not be NULL.
 * Run each shape once outside the capture first (scratch growth during a capture is refused with SPECKV_ERR_INVAL).
 * A plan names record addresses: plan again after an allocation of the batch was freed, re-created or migrated. */
size_t speckv_ext_attend_plan_bytes(uint32_t n_seq);
speckv_status_t speckv_ext_attend_batch_plan(uint32_t n_seq, const speckv_handle_t* handles, const uint32_t* pos_end,
                                             uint32_t max_pos_end, void* d_plan, size_t plan_bytes, void* stream);
speckv_status_t speckv_ext_attend_fp8_planned(const void* d_plan, uint32_t n_seq, uint32_t layer, const void* d_q_f16,
                                              uint32_t g, uint32_t max_pos_end, float sm_scale, float* d_out,
                                              float* d_lse, void* stream);
speckv_status_t speckv_ext_attend_int4_planned(const void* d_plan, uint32_t n_seq, uint32_t layer, const void* d_q_f16,
                                               uint32_t g, uint32_t max_pos_end, float sm_scale, float* d_out,
                                               float* d_lse, void* stream);

/* A planned layer AND the position the caller still holds outside the pool, in one call (round 6: the connector used to issue
 * speckv_ext_attend_fold_tail behind every layer's attention -- eight dependent launches of a few microseconds in an 8-layer step).
 *   scheme        SPECKV_COMP_FP8_E4M3 / _INT4_G32 / _MXFP4 (the plan's)
 *   n_tail        sequences of the batch that have such a position (0: exactly speckv_ext_attend_*_planned)
 *   d_tail_rows   device array [n_tail] of their indices in the batch (NULL when n_tail == n_seq: tail i belongs to sequence i)
 *   d_tail_idx    device array [n_seq]: index of the sequence's tail rows, < 0 = none (the inverse of d_tail_rows; may be NULL when
 *                 n_tail == n_seq, or altogether -- then the fold is a launch of its own, below)
 *   d_k_tail, d_v_tail  fp16 [n_tail][layers][heads][128] (the BASE of the arrays: `layer` selects the row), tails
 *                 tail_stride_elems (a multiple of 8, >= layers * heads * 128) apart;  d_lse is required
 * MXFP4 with d_tail_idx (or n_tail == n_seq) and no empty sequence in the plan: the attention kernel folds the position in itself,
 * in the epilogue of each sequence's first split -- no launch behind it.  Otherwise one k_attend_fold_tail launch follows inside the
 * call.  Either way the result is speckv_ext_attend_*_planned followed by speckv_ext_attend_fold_tail.  Capturable. */
speckv_status_t speckv_ext_attend_planned_tail(int scheme, const void* d_plan, uint32_t n_seq, uint32_t layer, const void* d_q_f16,
                                               uint32_t g, uint32_t max_pos_end, float sm_scale, float* d_out, float* d_lse,
                                               uint32_t n_tail, const uint32_t* d_tail_rows, const int32_t* d_tail_idx,
                                               const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride_elems, void* stream);

/* SEVERAL layers of a planned batch in one call, for callers that have the query rows of several layers at once (a draft model's
 * layers, a benchmark, layers whose attention inputs do not depend on each other): d_q_f16 [n_layers][n_seq][heads][g][128], d_out and
 * d_lse likewise; the tail arguments as speckv_ext_attend_planned_tail (n_tail == 0: none).  MXFP4 with a launch geometry of one split
 * per sequence (a batch that fills the chip by itself): ONE launch over layers x sequences -- the next layer's workgroups start while
 * the last of this one drain; everything else: the per-layer launches, issued from this one call.  Results equal the per-layer calls.
 * A tail stride shorter than (layer_begin + n_layers) * heads * 128 is refused with SPECKV_ERR_INVAL before anything is launched. */
speckv_status_t speckv_ext_attend_planned_layers(int scheme, const void* d_plan, uint32_t n_seq, uint32_t layer_begin, uint32_t n_layers,
                                                 const void* d_q_f16, uint32_t g, uint32_t max_pos_end, float sm_scale, float* d_out,
                                                 float* d_lse, uint32_t n_tail, const uint32_t* d_tail_rows, const int32_t* d_tail_idx,
                                                 const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride_elems, void* stream);

/* speckv_ext_attend_fold_tail: one more position for rows that already hold an attention result and its log-sum-exp
 * (speckv_ext_attend_* with d_lse) -- the fp16 K / V row a decode step produced but has not stored yet (pages hold
 * position PAIRS; a connector keeps the odd position until its partner arrives):
 *     s = q.k * sm_scale;  new = logaddexp(lse, s);  out = out * exp(lse - new) + v * exp(s - new);  lse = new
 *   d_rows   : device array of n_rows sequence indices into d_q_f16 / d_out / d_lse, or NULL for 0..n_rows-1
 *   d_q_f16  : [n_seq][heads][g][128] fp16      d_out : [n_seq][heads][g][128] fp32      d_lse : [n_seq][heads][g] fp32
 *   d_k_tail, d_v_tail : fp16 [n_rows][heads][128], consecutive rows tail_stride_elems (>= heads*128, even) apart
 * A sequence without stored positions (out = 0, lse = -inf from the batch call) ends as out = v, lse = s.
 * One launch, in place, capturable. */
speckv_status_t speckv_ext_attend_fold_tail(uint32_t n_rows, const uint32_t* d_rows, uint32_t heads, uint32_t g,
                                            const void* d_q_f16, const void* d_k_tail, const void* d_v_tail,
                                            uint64_t tail_stride_elems, float sm_scale, float* d_out, float* d_lse,
                                            void* stream);

/* speckv_ext_attend_fold_held: SEVERAL positions held outside the pool, folded causally -- the step of speculative decoding
 * (verify n_q draft positions of a sequence at once), of chunked prefill and of batches whose members advance by different counts.
 * The n_q query positions of a sequence ride through speckv_ext_attend_*_planned as g = n_q x rows_per_pos query rows per kv head
 * (row r belongs to query position j = r / rows_per_pos; every query position sees every stored position, so that pass needs no
 * mask); this entry then adds the fp16 K / V rows the caller still holds: d_base[i] positions in front of query position 0 (a
 * connector's odd last position: 0 or 1) followed by the new positions.  Query position j of sequence i folds held positions
 * 0 .. d_base[i] + j inclusive -- itself, not the drafts behind it -- each by the formula of speckv_ext_attend_fold_tail.
 *   d_rows   : device array of n_rows sequence indices into d_q_f16 / d_out / d_lse, or NULL for 0..n_rows-1 (held rows, d_base and
 *              d_n_q are indexed by i = 0..n_rows-1 either way)
 *   d_q_f16  : [n_seq][heads][g][128] fp16     d_out : the same in fp32     d_lse : [n_seq][heads][g] fp32, required
 *   g <= 16, a multiple of rows_per_pos;  n_q = g / rows_per_pos
 *   d_k_held, d_v_held : fp16, position t of sequence i at i * seq_stride_elems + t * pos_stride_elems + head * 128 elements (offset
 *              to the layer by the caller); both strides multiples of 8, pos_stride_elems >= heads * 128, seq_stride_elems >=
 *              (n_q - 1) * pos_stride_elems + heads * 128
 *   d_base   : device array [n_rows], d_base[i] + n_q <= SPECKV_HELD_MAX (the kernel reads no position past SPECKV_HELD_MAX - 1)
 *   d_n_q    : device array [n_rows] of live query positions per sequence, or NULL = n_q for all; rows of the positions >= d_n_q[i]
 *              are left exactly as they came in
 * A row without stored positions (out = 0, lse = -inf) ends as the softmax attention over its visible held positions;
 * d_base = 0 and n_q = 1 is speckv_ext_attend_fold_tail.  Bad arguments are SPECKV_ERR_INVAL before anything is launched.
 * ONE launch for all sequences, heads, rows and positions, in place, nothing allocated, capturable. */
#define SPECKV_HELD_MAX 17u              /* held positions per sequence: one left over + 16 new ones */
speckv_status_t speckv_ext_attend_fold_held(uint32_t n_rows, const uint32_t* d_rows, uint32_t heads, uint32_t g,
                                            uint32_t rows_per_pos, const void* d_q_f16, const void* d_k_held,
                                            const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems,
                                            const uint32_t* d_base, const uint32_t* d_n_q, float sm_scale, float* d_out,
                                            float* d_lse, void* stream);

/* speckv_ext_attend_fold_masked: speckv_ext_attend_fold_held with visibility from a MASK instead of a causal chain -- the step of a
 * speculative decoder that drafts a TREE (several continuations sharing a prefix; a node sees its ancestors, not its siblings).  The
 * pass over the stored positions is the same (every query row sees every stored position); only this fold differs.
 *   d_mask   : device array of 32-bit words; the word of sequence i (0..n_rows-1), query position j lies at i * mask_stride + j, with
 *              mask_stride >= n_q = g / rows_per_pos.  Bit t set = held position t of sequence i is visible to query position j; the
 *              visible positions are folded in ascending t, each by the formula of speckv_ext_attend_fold_tail.  Bits at or above
 *              SPECKV_HELD_MAX are ignored.  A word of 0 leaves the rows of that query position exactly as they came in (a dead node
 *              of a ragged step; the place of d_n_q).  The kernel reads no held position above the highest set bit of a word.
 *   everything else -- d_rows, d_q_f16, d_out, d_lse (required), g, rows_per_pos, the held rows and their strides, stream -- as
 *              speckv_ext_attend_fold_held.
 * A causal chain is the mask (1 << (d_base[i] + j + 1)) - 1, with 0 for the positions >= d_n_q[i]: with those words this entry
 * computes what speckv_ext_attend_fold_held computes.  Bad arguments (those speckv_ext_attend_fold_held refuses, a null d_mask,
 * mask_stride < n_q) are SPECKV_ERR_INVAL before anything is launched.
 * ONE launch for all sequences, heads, rows and positions, in place, nothing allocated, capturable. */
speckv_status_t speckv_ext_attend_fold_masked(uint32_t n_rows, const uint32_t* d_rows, uint32_t heads, uint32_t g,
                                              uint32_t rows_per_pos, const void* d_q_f16, const void* d_k_held,
                                              const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems,
                                              const uint32_t* d_mask, uint32_t mask_stride, float sm_scale, float* d_out,
                                              float* d_lse, void* stream);

/* ---- tier manager (CXLMemoryManager, cxl_memory_manager.h:40-90) ---------- */
speckv_status_t speckv_ext_promote_to_l1(speckv_handle_t handle, uint64_t offset_bytes);
speckv_status_t speckv_ext_demote_to_l3(speckv_handle_t handle, uint64_t offset_bytes);
/* Move the pool records of pages [first_page, first_page+n) to pool GPU
 * `target_pool` (index into SPECKV_POOL_DEVICES order): hipMemcpyPeerAsync over
 * xGMI on a side stream, page table re-pointed, old slots freed.  The reference's
 * promote/demote only flip a tier tag (cxl_memory_manager.cpp:130-194). */
speckv_status_t speckv_ext_migrate(speckv_handle_t handle, uint64_t first_page,
                                   uint64_t n_pages, uint32_t target_pool);

/* Seal an allocation: pack its records back to back (128-byte aligned, page order, one extent per pool GPU) and return the
 * worst-case 4 KiB slots to the pool.  Only the variable-length scheme gains (SPECKV_COMP_INT8_DELTA_RLE; for the others the
 * call is a no-op): the pool then holds what the reference only counts (CompressedData::compressed_size, the ratio statistics
 * of cache_engine.cpp:62-78), and the copy-engine fetch moves record bytes instead of slots.  Reads are unaffected (they go
 * through the page table); a later write or migration first unpacks the allocation into slots again, so seal sequences that
 * are parked in the pool, not ones a decode loop appends to.  *bytes_before / *bytes_after (optional): pool bytes the
 * allocation holds.  Synchronous.  The packed extents are allocated before the slots are released (the records move in one
 * pass), so the pool needs room for the packed size on top of the slots for the duration of the call: SPECKV_ERR_NOMEM
 * leaves the allocation as it was. */
speckv_status_t speckv_ext_compact(speckv_handle_t handle, uint64_t* bytes_before, uint64_t* bytes_after);

/* ---- statistics (Statistics structs: cxl_memory_manager.h:73-83,
 *      speculative_prefetcher.h:59-66, cache_engine.h:65-72, memory_allocator.h:42-48) */
typedef struct {
    uint64_t l1_hits, l1_misses, l2_hits, l2_misses, l3_accesses;
    uint64_t migrations_l1_to_l3, migrations_l3_to_l1;
    uint64_t total_prefetches, successful_prefetches, mispredictions;
    uint64_t total_compressions, total_decompressions;
    uint64_t compressed_bytes, original_bytes;
    uint64_t total_allocations, total_deallocations;
    uint64_t current_allocated_bytes, peak_allocated_bytes;
    uint64_t dma_submitted, dma_completed;
    uint64_t pool_bytes_reserved, cache_bytes_reserved;
    uint32_t prefetch_depth, compression_scheme, quant_mode, n_pool_devices;
    uint64_t pool_migrated_pages;
    uint64_t prefetch_dropped;      /* speckv_prefetch requests that could not be addressed (no geometry / binding) */
    uint64_t copy_engine_runs;      /* hipMemcpyPeerAsync runs issued by the copy-engine fetch */
    uint64_t copy_engine_bytes;     /* bytes they moved into local staging */
    /* pool occupancy (cache_engine.cpp:62-78 keeps compressed_size / ratio statistics; here they are bytes of HBM):
     * capacity ratio of the live data = written_pages * 4096 / pool_bytes_in_use */
    uint64_t pool_bytes_in_use;     /* record storage held by live allocations (slots, or packed extents once sealed) */
    uint64_t written_pages;         /* pages of live allocations that hold a record */
    uint64_t sealed_allocations;    /* live allocations packed by speckv_ext_compact */
    uint64_t compactions;           /* speckv_ext_compact calls that packed an allocation */
    uint64_t flat_decoder_fetches;  /* speckv_ext_fetch_range launches that took the flat-run decoder by themselves (sealed size or length samples) */
    uint64_t copied_pages;          /* records speckv_ext_copy_runs copied from allocation to allocation (pages never written included) */
} speckv_ext_stats_t;
/* The struct only ever grows at its end.  speckv_ext_stats() writes sizeof(speckv_ext_stats_t) of THIS header: a caller
 * compiled against an older header must use the sized form, which writes min(out_size, the library's size) bytes (fields
 * are never reordered, so a prefix is a valid older struct); bytes of the caller's buffer beyond the library's struct are
 * zero-filled (a caller built against a NEWER header reads zeros there); *written (optional) = bytes of real data; out_size < 8
 * is SPECKV_ERR_INVAL.
 * SPECKV_EXT_ABI_VERSION is bumped whenever a struct of this header grows or an entry point changes meaning;
 * speckv_ext_abi_version() returns the library's value (the Python binding refuses a mismatch).  The one exception is this
 * struct's growth at its end under the sized form above: copied_pages arrived with speckv_ext_copy_runs under version 6 (a
 * library without it answers a sized call with zeros there, a caller without it never sees it). */
#define SPECKV_EXT_ABI_VERSION 6u
uint32_t        speckv_ext_abi_version(void);
speckv_status_t speckv_ext_stats(speckv_ext_stats_t* out);
speckv_status_t speckv_ext_stats_sized(void* out, size_t out_size, size_t* written);

/* ---- address encodings of the reference, pure functions ----
 * speckv_ext_encode_virt_page : SpeckvAllocator::encode_virt_page, speckv_allocator.cpp:92-103
 *                               (req<<32)|(layer<<16)|(head<<8)|(pos<<1)|kind  (fields overlap, as there)
 * speckv_ext_rtl_prefetch_vaddr: prefetch_core.v:92-98,158  low 64 bits of {req,layer,8'd0,pos,1'b0}
 * speckv_ext_atu_translate    : ATU/TLB miss mapping, cache_engine.cpp:131-132, address_translation.cpp:85-90:
 *                               0x4000000000 + (va & 0xFFFFFFFFFFFF)  (the engine itself translates through
 *                               the HBM page table; this is kept for parity of logical ids only) */
uint64_t speckv_ext_encode_virt_page(uint32_t req_id, uint16_t layer, uint16_t head, uint32_t pos, uint8_t kind);
uint64_t speckv_ext_rtl_prefetch_vaddr(uint32_t req_id, uint16_t layer, uint32_t pos);
uint64_t speckv_ext_atu_translate(uint64_t virtual_addr);

/* ---- legacy 3-tier address space (CXLMemoryManager, src/cxl_memory/cxl_memory_manager.cpp:9-322, and the
 *      cxl_access policy of src/integration/memory_allocator.cpp:105-143) -------------
 * Pure host arithmetic on logical addresses: bump allocation (virt from 0x100000000; phys L1 0x8000000000,
 * L2 0x10000000000, L3 0x20000000000), translate, tier tags with LRU / hot (> 10 touches) promotion, page states,
 * statistics -- call for call what the reference's class returns, including deallocate() forgetting only the first
 * page.  No data moves here (none moves in the reference either); the HIP engine applies the same policy to real
 * slots.  tier: 0 L1_GPU_LOCAL, 1 L2_PREFETCH, 2 L3_CXL_POOL; state: 0 INVALID, 1 SHARED, 2 EXCLUSIVE, 3 MODIFIED. */
typedef struct speckv_ext_mm speckv_ext_mm_t;
typedef struct {
    uint64_t l1_hits, l1_misses, l2_hits, l2_misses, l3_accesses;
    uint64_t migrations_l1_to_l3, migrations_l3_to_l1;
    double   l1_hit_rate, l2_hit_rate;
} speckv_ext_mm_stats_t;
speckv_ext_mm_t* speckv_ext_mm_new(uint64_t l1_gb, uint64_t l2_gb, uint64_t l3_gb, uint64_t page_size);
void     speckv_ext_mm_delete(speckv_ext_mm_t* m);
uint64_t speckv_ext_mm_allocate(speckv_ext_mm_t* m, uint64_t size_bytes, uint32_t layer_id, int preferred_tier);
void     speckv_ext_mm_deallocate(speckv_ext_mm_t* m, uint64_t virtual_addr);
uint64_t speckv_ext_mm_translate(speckv_ext_mm_t* m, uint64_t virtual_addr);
int      speckv_ext_mm_is_in_cache(speckv_ext_mm_t* m, uint64_t virtual_addr, int tier);
int      speckv_ext_mm_promote_to_l1(speckv_ext_mm_t* m, uint64_t virtual_addr);
int      speckv_ext_mm_demote_to_l3(speckv_ext_mm_t* m, uint64_t virtual_addr);
void     speckv_ext_mm_invalidate_page(speckv_ext_mm_t* m, uint64_t virtual_addr);
void     speckv_ext_mm_mark_modified(speckv_ext_mm_t* m, uint64_t virtual_addr);
int      speckv_ext_mm_get_page_state(speckv_ext_mm_t* m, uint64_t virtual_addr);
void     speckv_ext_mm_update_access_tracking(speckv_ext_mm_t* m, uint64_t virtual_addr);
int      speckv_ext_mm_is_hot_page(speckv_ext_mm_t* m, uint64_t virtual_addr);
void     speckv_ext_mm_get_statistics(speckv_ext_mm_t* m, speckv_ext_mm_stats_t* out);
uint64_t speckv_ext_mm_cxl_access(speckv_ext_mm_t* m, uint64_t base_virtual_addr, uint64_t offset);

/* ---- pool placement: the one rule the engine places records by, as pure functions -------------
 * An allocation of n_pages striped over n_pool pool GPUs: page p lives on pool p % n_pool as record p / n_pool of
 * that pool's run; pool k holds ceil((n_pages - k) / n_pool) records.  (n_pool == 0 is treated as 1.) */
void     speckv_ext_placement(uint64_t n_pages, uint32_t n_pool, uint64_t page,
                              uint32_t* pool_index, uint64_t* record_index);
uint64_t speckv_ext_pool_shard_pages(uint64_t n_pages, uint32_t n_pool, uint32_t pool_index);

/* hard-coded per-layer ratio table and analytic throughput of the reference
 * (cache_engine.cpp:25-33,142-148,286-296) */
double speckv_ext_layer_compression_ratio(uint32_t layer_id);
/* width/8 * MHz/1000 * engines (cache_engine.cpp:291-296): 51.2 for the reference's defaults */
double speckv_ext_codec_model_throughput_gbps(uint32_t num_engines, double clock_mhz, uint32_t data_width_bits);

/* ---- the batch and planned forms for a SLIDING-WINDOW (local) layer ----------------------------------------------------------------
 * One new position per request for a whole batch, on a layer whose query sees its last `window` positions only (Mistral, Gemma 2 / 3,
 * gpt-oss interleave such layers with global ones).  The launches walk the window, not the context: never more than
 * ceil((window + 31) / 32) tiles of 32 positions per member, whatever its length.
 *
 * A member has length = q_pos + 1 positions, the step's own included: pos_end[i] = length & ~1 (even) of them are stored in the pool,
 * an odd length keeps its last position outside (the caller's tail), so q_pos[i] is pos_end[i] - 1 (the query's own position is the last
 * stored one) or pos_end[i] (it is the tail).  The query sees [lo, q_pos], lo = max(0, length - window), window >= 1; the tail -- which
 * the planned entries take as before -- and a step's own stored position are always visible.  speckv_ext_decode_window_range is the rule
 * as a pure function (the same body the engine fills its descriptors by; works without speckv_init): the member is walked from
 * begin = lo & ~31 with the first skip = lo - begin positions (0..31, odd or even) masked, over n_pages = (pos_end - begin) / 2 pages;
 * n_pages = 0 where lo == pos_end: window 1 with an odd length, or a length below 2 -- such a member is handled as one with pos_end = 0.
 * window = 0 in the range function: no window (begin = skip = 0).
 *
 *   speckv_ext_attend_batch_window        speckv_ext_attend_{fp8,int4,mx4}_batch under a window; `scheme` = the pool's format.  window = 0
 *       (q_pos is then not read), or a window that cuts no member's pool positions, issues exactly the launches of those entries.
 *   speckv_ext_attend_batch_plan_window   speckv_ext_attend_batch_plan under a window >= 1 (0: the plan of speckv_ext_attend_batch_plan); the buffer
 *       holds speckv_ext_attend_plan_window_bytes(n_seq) bytes: descriptors, dispatch order, then one skip count per sequence.
 *       speckv_ext_attend_{fp8,int4,mx4}_planned, _planned_tail and _planned_layers run over such a plan unchanged -- they find it by its
 *       buffer.  Grid and scratch of its launches are functions of (n_seq, max_pos_end, window): the tile bound is the smaller of the
 *       context's and the window's, and the kernel form is decided by the window being there, not by what it cuts in one step, so a
 *       captured launch stays valid while the lengths move inside max_pos_end.  (Whether the MXFP4 kernel folds the tails itself or a
 *       launch behind it does is decided by the plan the capture ran over -- a member without pool pages, or window 1, means the launch
 *       -- and a captured call keeps that choice; the results are the same either way, as with speckv_ext_attend_batch_plan.)  A caller
 *       with local and global layers keeps one plan buffer per window value beside the global one.
 * Placements: pools in a single run take the linear kernels; a batch with a striped or migrated member runs through the page tables
 * (the kernels by residue class have no mask for the head of a tile).  SPECKV_ERR_INVAL: a q_pos outside {pos_end - 1, pos_end}, a NULL
 * q_pos with window != 0, a buffer below speckv_ext_attend_plan_window_bytes, a capturing stream, and whatever the entries without a
 * window refuse. */
size_t speckv_ext_attend_plan_window_bytes(uint32_t n_seq);
speckv_status_t speckv_ext_attend_batch_plan_window(uint32_t n_seq, const speckv_handle_t* handles, const uint32_t* pos_end /* even, stored */,
                                                    const uint32_t* q_pos /* pos_end - 1 <= q_pos <= pos_end */, uint32_t window,
                                                    uint32_t max_pos_end, void* d_plan, size_t plan_bytes, void* stream);
speckv_status_t speckv_ext_attend_batch_window(int scheme, uint32_t n_seq, const speckv_handle_t* handles, uint32_t layer,
                                               const void* d_q_f16, uint32_t g, const uint32_t* pos_end, const uint32_t* q_pos,
                                               uint32_t window, float sm_scale, float* d_out, float* d_lse, void* stream);
speckv_status_t speckv_ext_decode_window_range(uint32_t length, uint32_t window, uint32_t* out_begin, uint32_t* out_skip,
                                               uint32_t* out_n_pages);

/* Launch-form switches (tests, measurement runs): the library reads its environment ONCE, at the first speckv_init / raw codec
 * call of the process; after that a form is changed by this call only.  Keys (= the SPECKV_<KEY> environment names, lower case):
 * attend_splits, attend_tiles_per_split, attend_general, tc_multipass, tc_scan (1 one workgroup, 2 one wave), tc_no_pre,
 * tc_no_split_tiles, td_one_pass, td_expand_per_element, flush_no_small, flush_small_words, predict_batch_path, wgs_per_cu, tc_batch_one_wg (many-tensor launches: one workgroup per tensor),
 * rounds_consecutive, fetch_sweep (speckv_ext_fetch_range: 1 a fetch over the same range as the allocation's previous one walks the other
 * way and keeps its stores in the Infinity Cache, 0 always ascending, 2 always descending, 3 as 1 with non-temporal stores; speckv_ext_fetch_sweep_next), remote_engine (1 kernel, 2 copy engines), copy_min_run_kb, slots_kind_fast (speckv_ext_read_slots / _write_slots:
 * the waves run (layer, kind) fastest instead of pair fastest), attend_stream (INT4_G32 / MXFP4, several layers of one
 * sequence: N > 0 the stream form in N pieces, -1 never), attend_mx4_one_half (MXFP4 batches: 4-wave workgroups also where
 * the two-halves form applies), attend_order_as_given (batches of members of different lengths: the caller's dispatch order), attend_fold_launch (speckv_ext_attend_planned_tail: the fold always as a launch of its own), attend_layers_loop
 * (speckv_ext_attend_planned_layers: always per-layer launches), attend_fp8_table_regs / attend_fp8_striped_table / attend_int4_striped_wg
 * (striped and migrated pools: the earlier kernel forms, kept as A/B partners and test coverage).  0 restores the library's own rule.
 * SPECKV_ERR_INVAL for an unknown key.  Works without speckv_init.  (INTEGRATION.md lists what each one does.) */
speckv_status_t speckv_ext_set_tuning(const char* key, long long value);

/* speckv_ext_codec_launch_shape: the shape the library gives a block-codec launch of n_blocks blocks (speckv_ext_codec_compress /
 * _decompress, the pool's writes and fetches, the flush and ring fetches) under the tuning in force -- the body the launchers
 * themselves call, as a pure function.  Workgroups have 4 waves.  Up to cap = n_cus x wgs_per_cu workgroups (tuning key wgs_per_cu,
 * 256 by default) a wave handles one block: *grid = ceil(n_blocks / 4), *per_wave = 1, *wave_step = 0.  Beyond that the launch has
 * rounds = ceil(ceil(n_blocks / 4) / cap) rounds: *per_wave = rounds blocks per wave and *grid = ceil(ceil(n_blocks / 4) / rounds)
 * <= cap.  Wave w of the launch (workgroup x 4 + wave) then handles the blocks w, w + *wave_step, ... below n_blocks, with
 * *wave_step = *grid x 4 (a round looks like a launch of its own), or, under the tuning key rounds_consecutive, the blocks
 * [w x *per_wave, min((w + 1) x *per_wave, n_blocks)) with *wave_step = 0.  Either way every block belongs to exactly one wave, also
 * when the device finds fewer blocks than the launch was sized for (the flush fetch).  n_blocks = 0: *grid = 1 (the launchers
 * launch nothing).  n_cus = 0: the compute units of the current device, or 256 without a device.  Works without speckv_init.
 * SPECKV_ERR_INVAL for a NULL output. */
speckv_status_t speckv_ext_codec_launch_shape(uint64_t n_blocks, uint32_t n_cus, uint32_t* grid, uint64_t* per_wave, uint64_t* wave_step);

/* speckv_ext_fetch_sweep_next: the direction in which speckv_ext_fetch_range walks the blocks of a kernel-path launch, and how it marks
 * its stores -- the body the engine itself calls, as a pure function.  A launch decodes every block of its range either way and writes
 * the same bytes; a descending one starts at the top of the range, and one that keeps its stores writes the destination with plain
 * instead of non-temporal stores, so that the lines stay in the Infinity Cache.  A range larger than that cache (256 MiB of records plus
 * destination) that is fetched again and again in ascending order finds nothing of itself on die; walked the other way every second
 * time, a sweep starts by overwriting what the one before it wrote last, and those lines never go to memory.  The engine keeps, per
 * allocation, its previous kernel-path fetch: prev_first, prev_n, prev_descending, prev_valid (0: none yet, or the handle was freed).
 * With the call's first / n, `capturing` (the stream is being captured into a graph) and mode (the tuning key fetch_sweep; < 0: the
 * value in force) it gives *out_descending, *out_keep_stores and the state after the call in out_state[4] = {first, n, descending, valid}:
 *   mode 1   the same (first, n) as the previous fetch and n <= 393 216 blocks (beyond that the plain stores cost more than the cache
 *            saves): the opposite direction, stores kept; anything else: ascending, non-temporal
 *   mode 0   ascending, non-temporal;  mode 2  descending, stores kept (tests and measurements force the other form)
 *   mode 3   the directions of mode 1 with non-temporal stores (measurements)
 *   capturing: ascending and non-temporal whatever the mode, and the state is returned as it came (a replayed graph cannot alternate)
 * speckv_ext_fetch_list, the copy-engine path of speckv_ext_fetch_range (which leaves the state alone) and the staged, ring and flush
 * fetches are always ascending and non-temporal.  Works without speckv_init.  SPECKV_ERR_INVAL for a NULL output or a mode above 3. */
speckv_status_t speckv_ext_fetch_sweep_next(uint64_t prev_first, uint64_t prev_n, uint32_t prev_descending, uint32_t prev_valid,
                                            uint64_t first, uint64_t n, int capturing, int mode, uint32_t* out_descending,
                                            uint32_t* out_keep_stores, uint64_t* out_state);

/* Is `stream` (a hipStream_t) being captured into a HIP graph right now?  The batch entry points and speckv_ext_attend_batch_plan
 * refuse such a stream; a caller that plans ahead (SpeckvKVConnector.append) asks first.  *out_capturing = 0 for the NULL stream.
 * SPECKV_ERR_DRIVER when the runtime does not know the stream (destroyed by its owner).  Works without speckv_init. */
speckv_status_t speckv_ext_stream_is_capturing(void* stream, int* out_capturing);

/* library identity: "hip" when built with the HIP data path */
const char* speckv_ext_backend(void);

/* speckv_ext_attend_chunk: causal attention of a CHUNK of new positions per sequence over everything the sequence holds, for any
 * chunk length, in ONE launch -- chunked prefill of a long prompt, the differing suffix behind a fork, a prompt continued after a
 * truncate.  The semantics are those of a speckv_ext_attend_*_planned pass followed by speckv_ext_attend_fold_held, without their
 * limits of 16 query rows per pass and SPECKV_HELD_MAX held positions.  Sequence i (allocation handles[i], shim layout with 8 kv
 * heads x 128) has pos_end[i] stored positions (even), one held odd last position if tail_idx[i] >= 0 (row tail_idx[i] of d_k_tail /
 * d_v_tail, tail_stride_elems apart) and n_q[i] <= C new positions: new position j, head h at d_k_new / d_v_new + i * seq_stride_elems
 * + j * pos_stride_elems + h * 128 elements (offset to the layer by the caller; read where they lie, no gathered copy).  Query
 * position j < n_q[i] sees the stored positions [0, pos_end[i]), the tail, the new positions in front of it and itself.
 *   d_q_f16 : [n_seq][C][heads][rows_per_pos][128] fp16, rows_per_pos in {1, 2, 4, 8, 16} query rows per kv head and position
 *   d_out   : the same in fp32: softmax(q.K^T sm_scale).V, normalised     d_lse : [n_seq][C][heads][rows_per_pos] fp32 natural-log
 *             sum of the exponentials, or NULL.  Rows of positions >= n_q[i] are not computed and not written.
 * Stored K and V enter as the fp16 values speckv_ext_fetch_range decodes for the page (a page never written: zeros; records at or
 * beyond pos_end[i], which a truncate leaves behind, are never seen).  THE QUERY STAYS fp16 for all three formats: unlike the FP8 and
 * MXFP4 decode kernels (speckv_ext_attend_fp8_* / _mx4_*), which quantise q, this entry does not.  Both products run on fp16 MFMA with
 * fp32 accumulation; the softmax weights are rounded to fp16.  There is no split over positions: a row's result does not depend on
 * which other sequences share the call.  One workgroup takes 64 / rows_per_pos positions of one kv head, so the call suits chunks;
 * a step of a few positions over a long context is spread wider by speckv_ext_attend_*_planned + speckv_ext_attend_fold_held.
 * One layer per call.  Asynchronous on `stream`; the host arrays are copied before return.  The records are read behind what the
 * caller queued on `stream` and behind the asynchronous pool writes handed to other streams before the call.  NOT capturable into a
 * HIP graph: the per-sequence descriptors are staged per call through a pinned slot (a capturing stream is SPECKV_ERR_INVAL).
 * Nothing is allocated once the descriptor slots exist; nothing in the pool or its caches changes.
 *   SPECKV_ERR_INVAL    NULL stream or arrays, an odd pos_end[i] or one beyond the layout, n_q[i] > C, C == 0, a bad rows_per_pos,
 *                       strides that are not multiples of 8 or shorter than heads * 128, pointers that are not 16-byte aligned, a
 *                       tail without tail rows, allocations of different schemes or of a scheme other than FP8_E4M3, INT4_G32,
 *                       MXFP4, a layout other than 8 x 128 fp16, a layer beyond the layout -- nothing is launched
 *   SPECKV_ERR_GENERAL  an unknown handle
 * n_seq == 0 or every n_q[i] == 0: SPECKV_OK, nothing is launched. */
speckv_status_t speckv_ext_attend_chunk(uint32_t n_seq, const speckv_handle_t* handles, uint32_t layer,
                                        const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                                        const uint32_t* pos_end, const uint32_t* n_q /* host arrays [n_seq] */,
                                        const void* d_k_new, const void* d_v_new, uint64_t seq_stride_elems,
                                        uint64_t pos_stride_elems,
                                        const int32_t* tail_idx /* host [n_seq], < 0 = none; may be NULL */,
                                        const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride_elems,
                                        float sm_scale, float* d_out, float* d_lse, void* stream);

/* speckv_ext_attend_chunk_masked: speckv_ext_attend_chunk for new positions that form a TREE of drafts of any size (no bound of 16
 * rows per pass or SPECKV_HELD_MAX held positions: a 64-node tree is one launch that reads the records once per 64 query rows).  The
 * arguments of speckv_ext_attend_chunk in the same order, with d_mask and mask_words in front of sm_scale; everything said there
 * holds -- layouts, the fp16 query, ordering, NOT capturable into a HIP graph, what is refused -- except what a row sees of the HELD
 * positions.  Those are numbered as the kernel walks them: held position 0 is the tail if sequence i has one (base = 1, else 0), new
 * position a is held position base + a.
 *   d_mask : device, uint32 [n_seq][C][mask_words]; the row of query position j of sequence i starts at d_mask + (i * C + j) *
 *            mask_words.  Bit t of the row (bit t & 31 of word t >> 5) = held position t is visible to it: the low `base` bits, then
 *            bits base + a -- the convention of speckv_ext_attend_fold_masked, continued over several words.  mask_words >=
 *            (C + 1 + 31) / 32; a larger row stride is fine, words beyond that are not read.
 *   The causal bound stays: held position t is seen iff t < base + j + 1 AND its bit is set, so bits at or beyond base + j + 1 are
 *   IGNORED.  Stored positions [0, pos_end[i]) are visible to every live row.
 *   A row is LIVE iff j < n_q[i] AND its own bit base + j is set.  A row that is not live is not computed and NOT WRITTEN (d_out and
 *   d_lse keep what they held), exactly like rows of positions >= n_q[i]; a live row always sees itself.
 * A chain (row j = the low base + j + 1 bits) gives speckv_ext_attend_chunk's result bit for bit.  The mask is read by the kernel in
 * place, behind what the caller queued on `stream`.
 *   SPECKV_ERR_INVAL    as speckv_ext_attend_chunk, and: d_mask NULL or not 4-byte aligned, mask_words < (C + 1 + 31) / 32 -- nothing
 *                       is launched
 *   SPECKV_ERR_GENERAL  an unknown handle */
speckv_status_t speckv_ext_attend_chunk_masked(uint32_t n_seq, const speckv_handle_t* handles, uint32_t layer,
                                               const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                                               const uint32_t* pos_end, const uint32_t* n_q /* host arrays [n_seq] */,
                                               const void* d_k_new, const void* d_v_new, uint64_t seq_stride_elems,
                                               uint64_t pos_stride_elems,
                                               const int32_t* tail_idx /* host [n_seq], < 0 = none; may be NULL */,
                                               const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride_elems,
                                               const uint32_t* d_mask, uint32_t mask_words,
                                               float sm_scale, float* d_out, float* d_lse, void* stream);

/* speckv_ext_attend_chunk_split: speckv_ext_attend_chunk / speckv_ext_attend_chunk_masked with the STORED positions of a sequence
 * split across the chip -- a step of a few positions, a small draft tree (of more than 16 nodes, which the decode entries refuse), a
 * fork's short suffix or a prompt's last short chunk over a LONG context, where the query blocks alone (8 kv heads x ceil(n_q /
 * (64 / rows_per_pos)) workgroups per sequence) leave most of the compute units idle.  ONE entry for the causal and the tree form: the
 * arguments of speckv_ext_attend_chunk_masked in the same order, with n_splits in front of sm_scale; d_mask == NULL is the causal
 * form (mask_words is then ignored).  Everything said at those two entries holds -- layouts, the fp16 query, liveness, rows that are
 * not live are NOT WRITTEN, ordering, NOT capturable into a HIP graph, what is refused.
 *   n_splits == 1 : every sequence whole.
 *   n_splits == N, 2 <= N <= SPECKV_CHUNK_SPLITS_MAX (forced): sequence i is cut into min(N, max(1, n_pool_i)) pieces, n_pool_i =
 *                   ceil(pos_end[i] / 32) pool tiles, evened out so that no piece is empty (speckv_ext_chunk_split_plan).
 *   n_splits == 0 : the library's rule (speckv_ext_chunk_split_plan): no pieces while the query blocks of the call fill the chip,
 *                   otherwise as many as still fit one round of three workgroups per compute unit, no piece under 32 pool tiles.
 * When the plan gives every sequence ONE piece, the call issues exactly the launch of speckv_ext_attend_chunk / _masked: no scratch,
 * no merge, the same output bits.  Otherwise it issues TWO launches on `stream`: the pieces (piece p of a sequence walks its share of
 * the pool tiles, the last piece also the held positions) write un-normalised partials to a scratch buffer of the engine, and a merge
 * combines a row's partials in ascending piece order (fp32; deterministic: the same call gives the same bits, whatever the
 * scheduling).  The buffer grows on demand to (sum of query blocks x pieces) x 8 x 33280 bytes and is kept; a call on another stream
 * than the previous split call's is ordered behind that call.
 * WITH n_splits != 1 A ROW'S BITS DEPEND ON THE PIECE COUNT of its sequence (another summation order; the values stay within the
 * entry's error bound).  Under n_splits == 0 the piece count depends on the WHOLE CALL -- the other sequences, their n_q,
 * rows_per_pos, the device -- so a row's bits may depend on which other sequences share the call.  A forced count depends on the
 * sequence alone (its pos_end), so under it a row's bits do not depend on its batch mates.
 *   SPECKV_ERR_INVAL    as speckv_ext_attend_chunk (and, with a mask, as speckv_ext_attend_chunk_masked: d_mask not 4-byte aligned,
 *                       mask_words < (C + 1 + 31) / 32), and n_splits > SPECKV_CHUNK_SPLITS_MAX -- nothing is launched
 *   SPECKV_ERR_NOMEM    the scratch buffer could not grow -- nothing is launched
 *   SPECKV_ERR_GENERAL  an unknown handle */
#define SPECKV_CHUNK_SPLITS_MAX 64u
speckv_status_t speckv_ext_attend_chunk_split(uint32_t n_seq, const speckv_handle_t* handles, uint32_t layer,
                                              const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                                              const uint32_t* pos_end, const uint32_t* n_q /* host arrays [n_seq] */,
                                              const void* d_k_new, const void* d_v_new, uint64_t seq_stride_elems,
                                              uint64_t pos_stride_elems,
                                              const int32_t* tail_idx /* host [n_seq], < 0 = none; may be NULL */,
                                              const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride_elems,
                                              const uint32_t* d_mask /* NULL: causal */, uint32_t mask_words, uint32_t n_splits,
                                              float sm_scale, float* d_out, float* d_lse, void* stream);

/* The piece rule of speckv_ext_attend_chunk_split as a pure function (the same body the entry calls): out_pieces[i] pieces of
 * out_tiles_per_piece[i] pool tiles (32 positions) for sequence i; piece p walks tiles [p * tpp, min((p + 1) * tpp, n_pool_i)), the
 * last piece also the held positions; a sequence without pool tiles has one piece of 0 tiles.
 *   n_splits == 1: one piece each.   n_splits == N > 1: pieces_i = min(N, max(1, n_pool_i)).
 *   n_splits == 0: G0 = 8 x the sum of ceil(n_q[i] / (64 / rows_per_pos)), target = 3 x n_cus (3 = resident workgroups per compute
 *   unit at the kernel's occupancy; n_cus == 0: the engine's device, 256 without an engine).  G0 >= target (or G0 == 0): one piece
 *   each; otherwise pieces_i = clamp(n_pool_i / 32, 1, min(floor(target / G0), SPECKV_CHUNK_SPLITS_MAX)): the pieces of a call fit
 *   one round of resident workgroups (so G0 > target / 2 is one piece each, too).
 *   Then tpp_i = ceil(n_pool_i / pieces_i) and pieces_i = ceil(n_pool_i / tpp_i): no piece is empty.
 * SPECKV_ERR_INVAL: NULL arrays with n_seq > 0, a rows_per_pos other than 1, 2, 4, 8, 16, n_splits > SPECKV_CHUNK_SPLITS_MAX.
 * Works without speckv_init. */
speckv_status_t speckv_ext_chunk_split_plan(uint32_t n_seq, const uint32_t* pos_end, const uint32_t* n_q, uint32_t rows_per_pos,
                                            uint32_t n_splits, uint32_t n_cus, uint32_t* out_pieces, uint32_t* out_tiles_per_piece);

/* speckv_ext_attend_chunk_window: speckv_ext_attend_chunk_split for a SLIDING-WINDOW (local) layer -- the models that interleave
 * local and global attention layers (the Mistral family, Gemma 2 / 3, gpt-oss) call this entry on their local layers and the other
 * chunk entries on their global ones.  The arguments of speckv_ext_attend_chunk_split in the same order with its two mask arguments
 * replaced by `window`; this entry has no tree form (a node's position in a tree is its depth, not its index: a draft tree on a
 * local layer goes to speckv_ext_attend_chunk_tree_window, at the end of this header).  Everything
 * said at speckv_ext_attend_chunk and speckv_ext_attend_chunk_split holds -- layouts, the fp16 query, rows of positions >= n_q[i] are
 * NOT WRITTEN, n_splits, ordering, NOT capturable into a HIP graph, what is refused -- except what a row sees.
 *   window == W >= 1 (one value for all sequences of the call): query position j of sequence i sits at the absolute position
 *            P = pos_end[i] + base + j (base = 1 with a tail, else 0) and sees the absolute positions [lo, P], lo = max(0, P + 1 - W):
 *            stored position t iff lo <= t < pos_end[i]; held position t (the tail is 0, new position a is base + a; its absolute
 *            position is pos_end[i] + t) iff pos_end[i] + t >= lo and t <= base + j.  Every live row sees itself.  W == 1 is a row
 *            that sees itself alone.  n_q[i] == 1 is the windowed DECODE step of a sequence of any length, odd or even.
 *   window == 0 : no window.
 * With window == 0, and with a window under which no row of the call loses a position (W >= pos_end[i] + base + n_q[i] for every
 * sequence with n_q[i] > 0), the call issues exactly the launches of speckv_ext_attend_chunk_split with d_mask == NULL: the same
 * output bits.  Otherwise the whole call runs on the window form of the kernel: a query block of 64 / rows_per_pos positions walks
 * only the 32-position tiles that hold a position one of its rows sees (speckv_ext_chunk_window_walk) -- never more than
 * ceil((W + 64 / rows_per_pos - 1) / 32) + 2 of them, whatever the sequence's length -- and positions no row of the block sees are
 * not read.  n_splits then cuts the pool tiles that are LEFT: from the first pool tile position 0 of the sequence sees
 * (floor(lo(0) / 32)) on, by the rule of speckv_ext_chunk_split_plan over that many tiles; a piece that lies wholly below a later
 * block's bound contributes nothing to it.  Records below a window stay in the pool as they are: nothing is freed or evicted.
 *   SPECKV_ERR_INVAL    as speckv_ext_attend_chunk, and n_splits > SPECKV_CHUNK_SPLITS_MAX -- nothing is launched
 *   SPECKV_ERR_NOMEM    the scratch buffer could not grow -- nothing is launched
 *   SPECKV_ERR_GENERAL  an unknown handle */
speckv_status_t speckv_ext_attend_chunk_window(uint32_t n_seq, const speckv_handle_t* handles, uint32_t layer,
                                               const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                                               const uint32_t* pos_end, const uint32_t* n_q /* host arrays [n_seq] */,
                                               const void* d_k_new, const void* d_v_new, uint64_t seq_stride_elems,
                                               uint64_t pos_stride_elems,
                                               const int32_t* tail_idx /* host [n_seq], < 0 = none; may be NULL */,
                                               const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride_elems,
                                               uint32_t window /* 0: none */, uint32_t n_splits,
                                               float sm_scale, float* d_out, float* d_lse, void* stream);

/* The walk rule of speckv_ext_attend_chunk_window as a pure function (the same body the kernel walks by).  Sequence i has pos_end[i]
 * (even) stored positions, base[i] in {0, 1} held tail positions (base == NULL: none) and n_q[i] new positions in query blocks of
 * per_blk = 64 / rows_per_pos positions; the kernel's tile index counts the n_pool = ceil(pos_end[i] / 32) pool tiles first, then the
 * held tiles.  Block blk (first position j_first = blk * per_blk, last live position j_last) walks the tiles [t_first, n_tiles):
 *   n_tiles = n_pool + ((base + j_last) >> 5) + 1
 *   t_first = lo >> 5 if lo < pos_end[i], else n_pool + ((lo - pos_end[i]) >> 5),  lo = max(0, pos_end[i] + base + j_first + 1 - window)
 * (window == 0: lo = 0).  out_first_tile / out_n_tiles: one entry per (sequence, block), the sequences in order and a sequence's
 * ceil(n_q[i] / per_blk) blocks in order -- t_first and n_tiles - t_first.
 * SPECKV_ERR_INVAL: NULL arrays with n_seq > 0, a rows_per_pos other than 1, 2, 4, 8, 16, an odd pos_end[i], base[i] > 1.
 * Works without speckv_init and needs no device. */
speckv_status_t speckv_ext_chunk_window_walk(uint32_t n_seq, const uint32_t* pos_end, const uint32_t* base /* may be NULL */,
                                             const uint32_t* n_q, uint32_t rows_per_pos, uint32_t window,
                                             uint32_t* out_first_tile, uint32_t* out_n_tiles);

/* speckv_ext_attend_prefix_fold: SHARED-PREFIX (cascade) attention -- the query rows of several requests attend the stored positions
 * of ONE other allocation, read once per 64 query rows and not once per request, and the result is FOLDED into what each request
 * attended on its own (parallel samples of one prompt, beams, a system prompt in front of many users).
 *   Group g (g < n_groups) = the prefix allocation prefix_handles[g] and the MEMBERS [first_member[g], first_member[g + 1]) of the
 *   call; first_member is a host array [n_groups + 1], ascending from 0; n_members = first_member[n_groups].  A member is a row of the
 *   caller's arrays, not an allocation: the library never learns which request it belongs to.
 *   d_q_f16 : device, fp16 [n_members][C][8 kv heads][rows_per_pos][128], 16-byte aligned -- the chunk entries' layout with the
 *             member in the place of the sequence; C == 1 is a decode step.  THE QUERY STAYS fp16 in all three formats.
 *   d_out   : device, fp32, the shape of d_q_f16, 16-byte aligned; d_lse : device, fp32 [n_members][C][8][rows_per_pos], natural
 *             log, REQUIRED.  Both are READ AND WRITTEN.
 *   prefix_len, n_q : host arrays [n_members].  Every live row of member m sees the stored positions [0, prefix_len[m]) of its
 *             group's prefix at `layer`; prefix_len[m] is even and at most the layout's num_tokens; two members of a group may see
 *             different lengths of the same prefix.  Member m brings n_q[m] <= C positions.  Nothing is held: no tail, no new rows,
 *             no causal structure among the rows.  A (member, position) pair with position >= n_q[m] or prefix_len[m] == 0 is DEAD:
 *             its q is not read and its out / lse rows are neither read nor written.
 * THE FOLD.  The call runs on `stream` behind the launches that wrote the members' own (out, lse) -- speckv_ext_attend_*_planned*
 * for a decode step, speckv_ext_attend_chunk* for a chunk -- and replaces them in place: with lse_p = ln sum exp(score) over the
 * prefix positions and out_p their normalised attention, new = logaddexp(lse, lse_p), out = out exp(lse - new) + out_p exp(lse_p -
 * new), lse = new: the softmax over the concatenation.  A member without positions of its own arrives as out = 0, lse = -inf (the
 * decode entries' result for an empty range) and leaves as exactly out_p, lse_p.
 *   n_splits : as speckv_ext_attend_chunk_split, over one "sequence" per group with pos_end = the largest prefix_len of the group's
 *             live members and n_q = members x C (speckv_ext_chunk_split_plan): 1 = one workgroup walks a group's tiles for 64 rows,
 *             N = that many pieces, 0 = the library's rule.  With pieces: a piece launch and a merge on `stream`, the partials in the
 *             library's scratch.  A row's bits depend on its group's piece plan and on nothing else of the call.
 * A block walks the tiles up to its group's largest prefix_len; between a member's prefix_len and that maximum lie records the
 * member does not see: they are weighed 0, so a NON-FINITE V row stored there gives NaN (0 x NaN).
 * Ordering as speckv_ext_attend_chunk; speckv_free of a prefix waits for `stream`.  NOT capturable into a HIP graph.
 *   SPECKV_OK           also for zero groups, zero members and no live pair -- nothing is launched
 *   SPECKV_ERR_INVAL    a NULL pointer (d_lse included), d_q_f16 / d_out not 16-byte aligned, rows_per_pos not 1, 2, 4, 8 or 16,
 *                       C == 0, an odd prefix_len or one beyond num_tokens, n_q[m] > C, first_member not ascending from 0, a prefix
 *                       without layout, a scheme other than FP8 / INT4_G32 / MXFP4 or mixed schemes, layer out of range,
 *                       n_splits > SPECKV_CHUNK_SPLITS_MAX, more work items than a launch indexes, a capturing stream -- nothing is launched
 *   SPECKV_ERR_NOMEM    the scratch buffer could not grow -- nothing is launched
 *   SPECKV_ERR_GENERAL  an unknown handle */
speckv_status_t speckv_ext_attend_prefix_fold(uint32_t n_groups, const speckv_handle_t* prefix_handles /* host [n_groups] */,
                                              const uint32_t* first_member /* host [n_groups + 1] */, uint32_t layer,
                                              const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                                              const uint32_t* prefix_len, const uint32_t* n_q /* host arrays [n_members] */,
                                              uint32_t n_splits, float sm_scale, float* d_out, float* d_lse, void* stream);

/* speckv_ext_attend_prefix_fold_window: speckv_ext_attend_prefix_fold on a SLIDING-WINDOW (local) layer, for decode steps, chunks
 * and draft trees -- the local layers of the models speckv_ext_attend_chunk_window names, whose members hold only their own positions
 * on EVERY layer.  The arguments of speckv_ext_attend_prefix_fold in the same order with `own_seen, d_depth, window` directly behind
 * n_q; everything said there holds except which prefix positions a row sees and which rows are live.
 *   Member m sees the stored positions [0, prefix_len[m]) of its group's prefix IN FRONT OF its own positions.
 *   own_seen : host array [n_members]; own_seen[m] = the number of the member's OWN positions its query position of depth 0 sees
 *             without a window, itself included: the member's length for a decode step after its position was appended,
 *             pos_end + base + 1 for a chunk or tree step.  0: the member holds nothing and the query is judged as sitting directly
 *             behind the prefix.
 *   d_depth  : device, uint32 [n_members][C], 4-byte aligned, may be NULL.  The row of position j of member m has depth
 *             d = d_depth[m * C + j] (a draft tree: the table speckv_ext_attend_chunk_tree_window takes) or, with NULL, d = j (a
 *             chain).  It sees own_seen[m] + d own keys; the own call (speckv_ext_attend_*_planned* under a window,
 *             speckv_ext_attend_chunk_window, speckv_ext_attend_chunk_tree_window) applies the window to those exactly as without
 *             a prefix -- the window is relative, the own call does not change.
 *   window   : W.  Of the prefix the row sees [lo, prefix_len[m]), lo = max(0, prefix_len[m] + own_seen[m] + d - W).  A row with
 *             lo >= prefix_len[m] (own_seen[m] + d >= W) sees nothing of the prefix and is DEAD like a pair beyond n_q[m]: its out /
 *             lse rows are neither read nor written.  Every live row sees position lo, so its sum is never 0.  W == 0: no window.
 * A group's blocks walk the 32-position tiles [first_tile, ceil(max_len / 32)) only (speckv_ext_prefix_window_walk); pages below
 * 32 first_tile are never read.  n_splits cuts the tiles that are LEFT by the rule of speckv_ext_chunk_split_plan, as
 * speckv_ext_attend_chunk_window does; a piece wholly below a row's lo or beyond its prefix_len weighs nothing, and the merge gives
 * the unsplit weights.
 * With window == 0, or a window under which no live row can lose a prefix position (prefix_len[m] + own_seen[m] + n_q[m] - 1 <= W
 * for every member with n_q[m] > 0 and prefix_len[m] > 0; a depth is below n_q[m]), the call issues exactly the launches of
 * speckv_ext_attend_prefix_fold -- the same bits -- and d_depth is not read.
 * Returns what speckv_ext_attend_prefix_fold returns (a capturing stream included), and SPECKV_ERR_INVAL for a NULL own_seen with
 * members and a d_depth that is not 4-byte aligned.  Every refusal comes before any launch and leaves out / lse untouched. */
speckv_status_t speckv_ext_attend_prefix_fold_window(uint32_t n_groups, const speckv_handle_t* prefix_handles /* host [n_groups] */,
                                                     const uint32_t* first_member /* host [n_groups + 1] */, uint32_t layer,
                                                     const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                                                     const uint32_t* prefix_len, const uint32_t* n_q, const uint32_t* own_seen /* host arrays [n_members] */,
                                                     const uint32_t* d_depth /* device, may be NULL */, uint32_t window /* 0: none */,
                                                     uint32_t n_splits, float sm_scale, float* d_out, float* d_lse, void* stream);

/* The walk rule of speckv_ext_attend_prefix_fold_window as a pure function (the same body the engine plans by).  A member of group
 * g = [first_member[g], first_member[g + 1]) COUNTS when n_q[m] > 0, prefix_len[m] > 0 and its depth-0 bound
 * lo0 = max(0, prefix_len[m] + own_seen[m] - window) (window == 0: 0) is below prefix_len[m]; depth 0 gives a member's lowest bound.
 *   out_first_tile[g] = (the minimum of lo0 over the members that count) >> 5
 *   out_n_tiles[g]    = ceil(max_len / 32) - out_first_tile[g], max_len = the largest prefix_len of the members that count
 * and 0 / 0 for a group without such a member (it has no blocks).  own_seen == NULL: zeros.
 * SPECKV_ERR_INVAL: NULL arrays where they are needed, first_member not ascending from 0, an odd prefix_len.
 * Works without speckv_init and needs no device. */
speckv_status_t speckv_ext_prefix_window_walk(uint32_t n_groups, const uint32_t* first_member /* [n_groups + 1] */,
                                              const uint32_t* prefix_len, const uint32_t* own_seen /* may be NULL */, const uint32_t* n_q,
                                              uint32_t window, uint32_t* out_first_tile, uint32_t* out_n_tiles /* [n_groups] */);

/* speckv_ext_attend_chunk_kv: the chunk attention over a SPLIT POOL ("K8V4") -- a request's K rows in an FP8_E4M3 allocation and its
 * V rows in an MXFP4 allocation of their own, read by ONE launch.  FP8 keys keep the score error of the FP8 pool (the decode-regime
 * error of the 4-bit pools is K's), MXFP4 values cost what V in 4 bits costs in every regime: 2048 + 1088 bytes per position pair,
 * 2.61 : 1 against fp16.  An additive entry: SPECKV_EXT_ABI_VERSION stays what it is.
 * The arguments: k_handles and v_handles (host arrays [n_seq]) in the place of `handles`, `layer`, then exactly the argument list of
 * speckv_ext_attend_chunk_tree_window (declared behind this entry, at the end of this header) from d_q_f16 on.  Everything said at
 * speckv_ext_attend_chunk and its forms holds -- the fp16 query, held positions, liveness, rows that are not live are NOT WRITTEN, ordering behind asynchronous pool writes, NOT capturable
 * into a HIP graph.  The forms, by argument:
 *   d_mask == NULL : the causal form; d_depth is ignored and `window` acts as at speckv_ext_attend_chunk_window.
 *   d_mask != NULL : the tree form (speckv_ext_attend_chunk_masked); with window != 0, d_depth is required and the call is
 *                    speckv_ext_attend_chunk_tree_window's (the window folded into the mask by the caller, applied by depth to the
 *                    stored positions by the library).
 *   n_splits       : as speckv_ext_attend_chunk_split, in every form.
 * Addressing.  Both allocations are read as arrays of REGIONS of num_tokens / 2 pages (num_tokens = the layout's): K of `layer` is
 * region `layer` of k_handles[i], V of `layer` is region `layer` of v_handles[i]; stored position p of the layer lies in page
 * layer * num_tokens / 2 + p / 2 of either.  (In an ordinary layout region r is layer r / 2, kind r % 2: a layout of
 * (num_tokens, n / 2 layers, 8, 128, 2) describes n such regions.)
 * Values.  A stored K element enters the score as the E4M3 value of its record, the page's block scale multiplies the score in fp32
 * -- exactly what speckv_ext_attend_chunk does over an FP8 pool.  A stored V element enters as the fp16 value speckv_ext_fetch_range
 * decodes from the MXFP4 record.  The query, the tail and the new rows stay fp16.  A page never written reads as zeros.
 *   SPECKV_ERR_INVAL    everything the chunk entries refuse (speckv_ext_attend_chunk, _masked, _split, _tree_window), and: k_handles or
 *                       v_handles NULL, a K allocation whose scheme is not SPECKV_COMP_FP8_E4M3, a V allocation whose scheme is not
 *                       SPECKV_COMP_MXFP4, a layout that is not 8 heads x 128 fp16 or whose num_tokens is odd, num_tokens that differ
 *                       between the two allocations of a sequence, pos_end[i] > num_tokens, (layer + 1) * num_tokens / 2 beyond
 *                       either allocation's pages, a capturing stream -- nothing is launched
 *   SPECKV_ERR_NOMEM    the scratch buffer of a split call could not grow -- nothing is launched
 *   SPECKV_ERR_GENERAL  an unknown handle
 * speckv_free of either allocation waits for `stream`. */
speckv_status_t speckv_ext_attend_chunk_kv(uint32_t n_seq, const speckv_handle_t* k_handles, const speckv_handle_t* v_handles,
                                           uint32_t layer, const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                                           const uint32_t* pos_end, const uint32_t* n_q /* host arrays [n_seq] */,
                                           const void* d_k_new, const void* d_v_new, uint64_t seq_stride_elems,
                                           uint64_t pos_stride_elems,
                                           const int32_t* tail_idx /* host [n_seq], < 0 = none; may be NULL */,
                                           const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride_elems,
                                           const uint32_t* d_mask /* NULL: causal */, uint32_t mask_words,
                                           const uint32_t* d_depth, uint32_t window /* 0: none */, uint32_t n_splits,
                                           float sm_scale, float* d_out, float* d_lse, void* stream);

/* speckv_ext_attend_prefix_fold_kv: SHARED-PREFIX attention over a SPLIT POOL ("K8V4", see speckv_ext_attend_chunk_kv) -- the prefix
 * of a group is a request of the split pool, its K rows in an FP8_E4M3 allocation and its V rows in an MXFP4 allocation of their own,
 * read once per 64 query rows of the group's members by ONE launch (or a piece launch and its merge) and folded into what each member
 * attended on its own.  An additive entry: SPECKV_EXT_ABI_VERSION stays what it is.
 * The arguments: k_handles and v_handles (host arrays [n_groups]) in the place of `prefix_handles`, then exactly the argument list of
 * speckv_ext_attend_prefix_fold_window from first_member on.  Everything said at speckv_ext_attend_prefix_fold and at
 * speckv_ext_attend_prefix_fold_window holds word for word -- the members, the fp16 query, d_out / d_lse READ AND WRITTEN, THE FOLD (a
 * member without positions of its own arrives as out = 0, lse = -inf), DEAD pairs, the walk to the group's largest prefix_len,
 * n_splits, own_seen / d_depth / window and which rows a window leaves live, ordering, NOT capturable into a HIP graph.
 *   own_seen : may be NULL iff window == 0 (nothing reads it then).
 *   window   : 0, or a window that cuts nothing by the rule stated at speckv_ext_attend_prefix_fold_window, issues the unwindowed
 *              launches and their bits; d_depth is not read then.
 * Addressing.  As speckv_ext_attend_chunk_kv: both allocations are arrays of REGIONS of num_tokens / 2 pages, K of `layer` is region
 * `layer` of k_handles[g], V of `layer` is region `layer` of v_handles[g]; stored position p of the layer lies in page
 * layer * num_tokens / 2 + p / 2 of either.
 * Values.  A stored K element enters the score as the E4M3 value of its record, the page's block scale multiplies the score in fp32
 * -- exactly what speckv_ext_attend_prefix_fold does over an FP8 pool.  A stored V element enters as the fp16 value
 * speckv_ext_fetch_range decodes from the MXFP4 record.  The query stays fp16.  A page never written reads as zeros.
 *   SPECKV_OK           also for zero groups, zero members and no live pair -- nothing is launched
 *   SPECKV_ERR_INVAL    everything speckv_ext_attend_prefix_fold_window refuses (a NULL own_seen with members only where window != 0),
 *                       and: k_handles or v_handles NULL, a K allocation whose scheme is not SPECKV_COMP_FP8_E4M3, a V allocation whose
 *                       scheme is not SPECKV_COMP_MXFP4, a layout that is not 8 heads x 128 fp16 or whose num_tokens is odd, num_tokens
 *                       that differ between the two allocations of a group, prefix_len[m] > num_tokens, (layer + 1) * num_tokens / 2
 *                       beyond either allocation's pages, layer >= 2 * num_layers, a capturing stream -- nothing is launched
 *   SPECKV_ERR_NOMEM    the scratch buffer of a split call could not grow -- nothing is launched
 *   SPECKV_ERR_GENERAL  an unknown handle
 * Every refusal comes before any launch and leaves out / lse untouched.  speckv_free of either allocation waits for `stream`. */
speckv_status_t speckv_ext_attend_prefix_fold_kv(uint32_t n_groups, const speckv_handle_t* k_handles,
                                                 const speckv_handle_t* v_handles /* host [n_groups] */,
                                                 const uint32_t* first_member /* host [n_groups + 1] */, uint32_t layer,
                                                 const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                                                 const uint32_t* prefix_len, const uint32_t* n_q,
                                                 const uint32_t* own_seen /* host [n_members]; may be NULL iff window == 0 */,
                                                 const uint32_t* d_depth /* device, may be NULL */, uint32_t window /* 0: none */,
                                                 uint32_t n_splits, float sm_scale, float* d_out, float* d_lse, void* stream);

/* speckv_ext_attend_kv_batch: one DECODE STEP of a batch over a SPLIT POOL ("K8V4", see speckv_ext_attend_chunk_kv) -- the fused
 * attention of ONE layer for n_seq sequences over the stored positions [0, pos_end[i]), one new position per sequence with g query rows
 * per kv head, in one attention launch (and a merge launch where sequences are cut into pieces).  The decode-shaped counterpart of
 * speckv_ext_attend_chunk_kv, whose 64-row query blocks carry 1..16 live rows in a decode step and decode every tile to fp16 for them:
 * here K feeds v_mfma_f32_16x16x32_fp8_fp8 as it lies in the FP8 record and V is widened from the MXFP4 record in registers
 * (v_cvt_scalef32_pk_f16_fp4), no fp16 K or V is materialised.  An additive entry: SPECKV_EXT_ABI_VERSION stays what it is.
 *   k_handles, v_handles, pos_end : host arrays of n_seq      d_q_f16 : [n_seq][8][g][128] fp16 (device, 16-byte aligned)
 *   d_out : [n_seq][8][g][128] fp32 (16-byte aligned)         d_lse : optional [n_seq][8][g] fp32 log-sum-exp of the scaled scores
 * Shapes and stream rules are those of speckv_ext_attend_fp8_batch: g = 1..16, asynchronous on `stream` (the host arrays are copied
 * before the call returns; NULL = the engine's stream and a synchronous call), calls on several streams are ordered by the library
 * (one scratch buffer for the partials).  The call is ordered behind the asynchronous pool writes on every caller stream the engine
 * knows.  A sequence with pos_end[i] == 0 gets zeros and lse = -inf; a position the connector still holds outside the pool (an odd
 * length) is folded in afterwards by speckv_ext_attend_fold_tail, which is why a caller with such sequences passes d_lse.
 * The entry only reads, so a pair may appear many times in one call (each time with its own pos_end and query rows).
 * Addressing.  As speckv_ext_attend_chunk_kv: both allocations are arrays of REGIONS of num_tokens / 2 pages, K of `layer` is region
 * `layer` of k_handles[i], V of `layer` region `layer` of v_handles[i]; stored position p lies in page layer * num_tokens / 2 + p / 2.
 * Values.  The query is quantised by the kernel to E4M3 x a row scale (max|q| / 448 over the row, 1 for a zero row) exactly as
 * speckv_ext_attend_fp8_batch does.  A stored K element enters the score as the E4M3 value of its record, the page's block scale
 * multiplies the score in fp32.  A stored V element enters as the fp16 value speckv_ext_fetch_range decodes from the MXFP4 record; the
 * softmax weights meet it in fp16, accumulation is fp32.  A page never written reads as zeros: its positions score 0 (not -inf).
 * Placement.  ONE form: the records of both allocations of every sequence lie in a single run of one pool (what an engine with one
 * pool gives every allocation).  Striped and migrated placements are served by speckv_ext_attend_chunk_kv only.
 * The per-call descriptors travel through a pinned slot that later calls reuse: NOT capturable into a HIP graph.
 *   SPECKV_ERR_INVAL    k_handles, v_handles, pos_end, d_q_f16 or d_out NULL (with n_seq != 0), d_q_f16 or d_out not 16-byte aligned,
 *                       g == 0 or g > 16, a K allocation whose scheme is not SPECKV_COMP_FP8_E4M3, a V allocation whose scheme is not
 *                       SPECKV_COMP_MXFP4, a layout that is not 8 heads x 128 fp16 or whose num_tokens is not a multiple of 32,
 *                       num_tokens that differ between the two allocations of a sequence, pos_end[i] odd or > num_tokens,
 *                       (layer + 1) * num_tokens / 2 beyond either allocation's pages, an allocation whose records do not lie in one
 *                       run (the error text names the sequence), a member in more than 2048 pieces (the merge takes 2048 partials a
 *                       row at most; the library's own split rule stays far below, a forced attend_tiles_per_split may not), a
 *                       capturing stream -- nothing is launched, d_out is untouched
 *   SPECKV_ERR_NOMEM    the scratch buffer of the partials could not grow -- nothing is launched
 *   SPECKV_ERR_GENERAL  an unknown handle
 *   SPECKV_ERR_DRIVER   an engine without a device ("/dev/null"): no data path
 * speckv_free of either allocation waits for `stream`. */
speckv_status_t speckv_ext_attend_kv_batch(uint32_t n_seq, const speckv_handle_t* k_handles, const speckv_handle_t* v_handles,
                                           uint32_t layer, const void* d_q_f16, uint32_t g, const uint32_t* pos_end,
                                           float sm_scale, float* d_out, float* d_lse, void* stream);

/* speckv_ext_attend_kv_batch_window: speckv_ext_attend_kv_batch on a SLIDING-WINDOW (local) layer -- the decode step of the local layers
 * of a model that interleaves local and global attention (Mistral, Gemma 2 / 3, gpt-oss) over a split pool.  The arguments of
 * speckv_ext_attend_kv_batch with `q_pos, window` directly behind pos_end.  An additive entry: SPECKV_EXT_ABI_VERSION stays what it is.
 *   pos_end, q_pos, window : the semantics of speckv_ext_attend_batch_window.  Member i has length = q_pos[i] + 1 positions, the step's
 *       own included; pos_end[i] = length & ~1 of them are stored, so q_pos[i] is pos_end[i] - 1 (the query's own position is the last
 *       stored one) or pos_end[i] (it is the tail the caller holds; with pos_end[i] == 0 only q_pos[i] == 0).  The query sees the stored
 *       positions [lo, pos_end[i]), lo = max(0, length - window); speckv_ext_decode_window_range is the rule.  Each member is walked
 *       from the tile of lo in BOTH allocations -- at most ceil((window + 31) / 32) tiles whatever its context -- with the positions of
 *       that tile in front of lo masked (k_attend_k8v4<true>); the dispatch order and the pieces are decided on the pages walked.
 *   window = 0 (q_pos is then not read), or a window that cuts no member's pool positions: exactly the launches of
 *       speckv_ext_attend_kv_batch -- the same kernel instance, the same bits.
 *   A member without a pool position in its window (window 1 with an odd length, a length below 2) is handled as one with
 *       pos_end[i] == 0: zeros and lse = -inf.
 * Values, addressing, placement (single runs only), stream rules and statuses are those of speckv_ext_attend_kv_batch; the tail of an odd
 * length is always inside the window and is folded in afterwards by speckv_ext_attend_fold_tail, as there.  NOT capturable into a HIP
 * graph.  SPECKV_ERR_INVAL besides what speckv_ext_attend_kv_batch refuses: a q_pos[i] outside {pos_end[i] - 1, pos_end[i]}, a NULL
 * q_pos with window != 0 -- nothing is launched, d_out is untouched. */
speckv_status_t speckv_ext_attend_kv_batch_window(uint32_t n_seq, const speckv_handle_t* k_handles, const speckv_handle_t* v_handles,
                                                  uint32_t layer, const void* d_q_f16, uint32_t g, const uint32_t* pos_end,
                                                  const uint32_t* q_pos, uint32_t window, float sm_scale, float* d_out, float* d_lse,
                                                  void* stream);

/* speckv_ext_attend_kv_spec: one MULTI-POSITION STEP of a batch over a SPLIT POOL -- verifying the draft positions of every sequence, a
 * chain or a tree, on the decode kernel: speckv_ext_attend_kv_batch with g = n_q x rows_per_pos query rows per kv head (row r belongs to
 * query position j = r / rows_per_pos, n_q <= SPECKV_HELD_MAX - 1), every row over all stored positions [0, pos_end[i]) in ONE pass over
 * the records, and the positions the caller holds OUTSIDE the pool folded in INSIDE the same launch -- by the workgroups of a sequence's
 * first piece, into its final rows or its partial; the merge then runs as in speckv_ext_attend_kv_batch.  No fold launch follows; what
 * speckv_ext_attend_kv_batch + speckv_ext_attend_fold_masked compute in two calls.  An additive entry: SPECKV_EXT_ABI_VERSION stays what it is.
 *   k_handles, v_handles, layer, d_q_f16 ([n_seq][8][g][128] fp16), g, pos_end, sm_scale, d_out, d_lse (optional), stream :
 *       as speckv_ext_attend_kv_batch
 *   d_k_held, d_v_held : the held positions, fp16, the layout of speckv_ext_attend_fold_held: position t of sequence i, kv head h, at
 *       element i * seq_stride_elems + t * pos_stride_elems + h * 128 (the pointers already offset to the layer).  Held position 0 is the
 *       sequence's odd last position where it has one, the step's new positions follow; at most SPECKV_HELD_MAX per sequence.  Device
 *       pointers, 16-byte aligned; both strides multiples of 8, pos_stride_elems >= 8 * 128.
 *   d_mask, mask_stride : device array, d_mask[i * mask_stride + j] = the held positions query position j of sequence i sees, bit t =
 *       position t (the convention of speckv_ext_attend_fold_masked; bits >= SPECKV_HELD_MAX are dropped).  A causal chain behind `base`
 *       earlier held positions is the word (1 << (base + j + 1)) - 1: one form for chains and trees.  mask_stride >= g / rows_per_pos; a
 *       later group of a step that goes in several calls passes d_mask + its first position.
 *       The kernel reads NO held position above the highest bit set in any word of the sequence: such rows may hold anything.
 *       A word of 0 is a dead node of a ragged step: its rows leave as the attention over the stored positions alone (what
 *       speckv_ext_attend_kv_batch writes there), zeros and lse = -inf where nothing is stored.
 * Values.  The stored part as speckv_ext_attend_kv_batch (query as E4M3 x a row scale, K as its E4M3 values with the block scale on the
 * score, V as the fp16 values of its MXFP4 records).  A held position is scored with the FP16 query -- the fp32 sum of the products
 * over the 128 channels, x sm_scale -- and its fp16 V row is weighted in fp32; it enters the same running softmax as the stored tiles.
 * A sequence with pos_end[i] == 0 gets the softmax over its visible held positions.
 * Addressing, placement (single runs only), stream rules, ordering behind pool writes and statuses are those of
 * speckv_ext_attend_kv_batch.  NOT capturable into a HIP graph.  The form under a sliding window (a draft step on a local
 * layer) is speckv_ext_attend_kv_spec_window, below.  SPECKV_ERR_INVAL besides what speckv_ext_attend_kv_batch refuses, judged before anything
 * else and on every engine: rows_per_pos == 0, g not a multiple of rows_per_pos, g / rows_per_pos > SPECKV_HELD_MAX - 1, a NULL
 * d_k_held, d_v_held or d_mask, mask_stride < g / rows_per_pos, a stride that is not a multiple of 8, pos_stride_elems < 8 * 128, a held
 * pointer that is not 16-byte aligned -- nothing is launched, d_out is untouched. */
speckv_status_t speckv_ext_attend_kv_spec(uint32_t n_seq, const speckv_handle_t* k_handles, const speckv_handle_t* v_handles,
                                          uint32_t layer, const void* d_q_f16, uint32_t g, uint32_t rows_per_pos, const uint32_t* pos_end,
                                          const void* d_k_held, const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems,
                                          const uint32_t* d_mask, uint32_t mask_stride, float sm_scale, float* d_out, float* d_lse /* optional */,
                                          void* stream);

/* speckv_ext_attend_kv_spec_window: speckv_ext_attend_kv_spec on a SLIDING-WINDOW (local) layer -- the draft step of the local layers of
 * models that interleave local and global attention, on the decode kernel and in ONE launch as well.  The arguments of
 * speckv_ext_attend_kv_spec in the same order with `length, d_depth, window` directly behind pos_end.  An additive entry:
 * SPECKV_EXT_ABI_VERSION stays what it is.
 *   length  : host array, length[i] = the committed positions of sequence i, pos_end[i] (even) or pos_end[i] + 1 (the odd last position is
 *       held position 0).  The step's new positions follow: a node of depth d sits at the absolute position length[i] + d.
 *   d_depth : device array strided like d_mask, d_depth[i * mask_stride + j] = the depth of query position j of sequence i in the step's
 *       tree (0 = a root; a chain: j); depths above 15 are taken as 15.  A later group of a step passes d_depth + its first position, as it
 *       passes d_mask + it.
 *   window  : W >= 1.  A node of depth d sees the absolute positions [lo(d), length[i] + d], lo(d) = max(0, length[i] + d + 1 - W).  Of the
 *       STORED positions that is [lo(d), pos_end[i]), applied by the kernel PER QUERY ROW; what the node sees of the HELD positions (the
 *       odd last position, its ancestors, itself) is the caller's to say in d_mask, as ever: the window clears the bits of held positions
 *       in front of lo(d).
 * The walk (speckv_ext_spec_window_range is the rule as a pure function): each member is walked from the tile of DEPTH 0's bound,
 * begin = lo(0) & ~31, in both allocations, whatever depths the call carries -- a later group pays one extra, partly masked tile at most
 * -- over n_pages = (pos_end[i] - begin) / 2 pages, at most ceil((W + 31) / 32) tiles whatever the length; pieces and dispatch order are
 * decided on the pages walked.  Row r of depth d is masked over the leading skip = max(0, rel + d) <= 46 positions of the walk, rel =
 * length[i] + 1 - W - begin (signed): a row may see nothing of a tile or of a whole piece and still comes out right.  A member no row of
 * which sees a stored position (lo(0) >= pos_end[i]) is handled as one with nothing stored: its held positions alone; a row that sees
 * nothing anywhere is zeros with lse = -inf.
 * window == 0, or a window that can cut no member (length[i] + 16 <= window for every i): exactly the launches and the bits of
 * speckv_ext_attend_kv_spec; with window == 0 neither length nor d_depth is read.
 * Values, addressing, placement, stream rules and statuses are those of speckv_ext_attend_kv_spec.  NOT capturable into a HIP graph.
 * SPECKV_ERR_INVAL besides what speckv_ext_attend_kv_spec refuses, judged before anything else and on every engine: a NULL length or
 * d_depth with window != 0, a length[i] outside {pos_end[i], pos_end[i] + 1} -- nothing is launched, d_out is untouched. */
speckv_status_t speckv_ext_attend_kv_spec_window(uint32_t n_seq, const speckv_handle_t* k_handles, const speckv_handle_t* v_handles,
                                                 uint32_t layer, const void* d_q_f16, uint32_t g, uint32_t rows_per_pos, const uint32_t* pos_end,
                                                 const uint32_t* length, const uint32_t* d_depth, uint32_t window, const void* d_k_held,
                                                 const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems, const uint32_t* d_mask,
                                                 uint32_t mask_stride, float sm_scale, float* d_out, float* d_lse /* optional */, void* stream);

/* The walk rule of speckv_ext_attend_kv_spec_window as a pure function (works without speckv_init, needs no device): for a member of
 * `length` committed positions under window W >= 1, *out_begin = the first position walked (a multiple of 32), *out_n_pages = the pages
 * walked from there (0: no row sees a stored position), *out_rel = length + 1 - W - begin, signed -- a row of depth d does not see the
 * leading max(0, rel + min(d, 15)) positions of the walk.  SPECKV_ERR_INVAL: a NULL out pointer, window == 0. */
speckv_status_t speckv_ext_spec_window_range(uint32_t length, uint32_t window, uint32_t* out_begin, int32_t* out_rel, uint32_t* out_n_pages);

/* speckv_ext_attend_chunk_tree_window: a DRAFT TREE on a SLIDING-WINDOW (local) layer -- the tree step of the local layers of the
 * models speckv_ext_attend_chunk_window names, whose global layers take the tree step through speckv_ext_attend_chunk_masked / _split.
 * The arguments of speckv_ext_attend_chunk_split in the same order with `d_depth, window` directly behind mask_words.  Everything
 * said at speckv_ext_attend_chunk_masked and speckv_ext_attend_chunk_split holds -- layouts, the fp16 query, the numbering of the
 * held positions, liveness (j < n_q[i] AND the row's own bit), rows that are not live are NOT WRITTEN, n_splits, ordering, NOT
 * capturable into a HIP graph, what is refused -- except what a live row sees of the STORED positions.
 *   Sequence i holds length = pos_end[i] + base positions (base = 1 with a tail, else 0) and brings a tree of new nodes; node j has
 *   depth(j) = 0 where its parent is the committed context, else depth(parent) + 1, and sits at the absolute position
 *   P_j = length + depth(j).  Under window == W >= 1 it sees the absolute positions [lo_j, P_j] ON ITS OWN ROOT PATH,
 *   lo_j = max(0, P_j + 1 - W):
 *     stored position t  iff lo_j <= t < pos_end[i];
 *     the tail           iff base == 1 and pos_end[i] >= lo_j;
 *     ancestor a         iff length + depth(a) >= lo_j, i.e. depth(a) > depth(j) - W;
 *     itself             always (W == 1: the node's own V row).
 *   d_depth : device, uint32 [n_seq][C]; d_depth[i * C + j] = depth(j).  4-byte aligned; read by the kernel in place.
 *   d_mask  : as speckv_ext_attend_chunk_masked, with the window ALREADY FOLDED IN by the caller: of the held positions (tail,
 *             ancestors, itself) a row's bits keep those the rules above let it see.
 * THE LIBRARY APPLIES THE WINDOW TO THE STORED POSITIONS ONLY, by d_depth.  The held part is exactly what d_mask says -- the kernel
 * applies no lower bound there -- so d_mask and d_depth MUST COME FROM THE SAME TREE (SpeckvKVConnector.chunk_tree_masks(window=W)
 * and chunk_tree_depths build the pair).  There is no causal form: d_mask == NULL is refused.
 * The library cannot read the device arrays.  With window == 0, and with a window no node can lose a position under
 * (pos_end[i] + base + n_q[i] <= W for every sequence: a depth is below n_q[i]), the call issues exactly the launches of
 * speckv_ext_attend_chunk_split with this mask: the same output bits, d_depth is not read.  Otherwise the whole call runs on the
 * tree-window form of the kernel: every query block of a sequence walks the pool tiles from floor(lo(depth 0) / 32) on (depths are
 * not ordered by node index, so nothing is derived from a block's first row), then all held tiles as the masked form does; n_splits
 * cuts the pool tiles that are left by the rule of speckv_ext_chunk_split_plan, as speckv_ext_attend_chunk_window does.  A chain
 * given as a tree (parent j - 1, depth j) gives what speckv_ext_attend_chunk_window gives within the entry's error bound, not bit
 * for bit.  Records below a window stay in the pool: nothing is freed.
 *   SPECKV_ERR_INVAL    as speckv_ext_attend_chunk_split, and: d_mask or d_depth NULL or not 4-byte aligned, mask_words <
 *                       (C + 1 + 31) / 32 -- nothing is launched
 *   SPECKV_ERR_NOMEM    the scratch buffer could not grow -- nothing is launched
 *   SPECKV_ERR_GENERAL  an unknown handle */
speckv_status_t speckv_ext_attend_chunk_tree_window(uint32_t n_seq, const speckv_handle_t* handles, uint32_t layer,
                                                    const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                                                    const uint32_t* pos_end, const uint32_t* n_q /* host arrays [n_seq] */,
                                                    const void* d_k_new, const void* d_v_new, uint64_t seq_stride_elems,
                                                    uint64_t pos_stride_elems,
                                                    const int32_t* tail_idx /* host [n_seq], < 0 = none; may be NULL */,
                                                    const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride_elems,
                                                    const uint32_t* d_mask, uint32_t mask_words,
                                                    const uint32_t* d_depth, uint32_t window /* 0: none */, uint32_t n_splits,
                                                    float sm_scale, float* d_out, float* d_lse, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPECKV_EXT_H */
