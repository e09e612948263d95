// cxl-speckv_amd/csrc/page_table_kernels.inl -- page-table upkeep: k_apply_updates (flag / slot mirror), k_init_entries, and their
// launchers.
//
// A section of the translation unit kernels.hip, which includes it inside namespace speckv at the place where the text stood (why
// it is not a translation unit of its own yet: see there).  As one it would need kernels.hpp (PageEntry, DevAlloc, MirrorUpdate,
// kKeepSlot, kPlanarMx4, mx4_nib_off, mx4_code_delta) and nothing of kernels.hip or codec_device.hpp.  k_repack,
// k_retarget_entries and k_copy16 belong here by subject and are still in kernels.hip: see the note there.

namespace {

__global__ void k_apply_updates(const DevAlloc* __restrict__ tab, const MirrorUpdate* __restrict__ up, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const MirrorUpdate u = up[i];
    const DevAlloc t = tab[u.alloc_idx];
    if (!t.entries) return;
    if (u.and_mask != 0xFFFFFFFFu) atomicAnd(&t.d_flags[u.page], u.and_mask);
    if (u.or_mask) atomicOr(&t.d_flags[u.page], u.or_mask);
    if (u.slot != kKeepSlot) t.d_slot[u.page] = u.slot;
}

__global__ void k_init_entries(PageEntry* e, uint64_t n, uint64_t base, uint64_t stride, uint64_t rec0)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (stride == kPlanarMx4) { e[i].pool_addr = base + mx4_nib_off(rec0 + i); e[i].rec_bytes = 0; e[i].scale = __uint_as_float(mx4_code_delta(rec0 + i)); }
    else { e[i].pool_addr = base + i * stride; e[i].rec_bytes = 0; e[i].scale = 1.0f; }
}

} // namespace

hipError_t launch_apply_updates(const DevAlloc* d_tab, const MirrorUpdate* d_updates, uint32_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_apply_updates, dim3((n + 255u) / 256u), dim3(256), 0, s, d_tab, d_updates, n);
    return hipGetLastError();
}

hipError_t launch_init_entries(PageEntry* d_entries, uint64_t n, uint64_t base, uint64_t stride,
                               hipStream_t s, uint64_t rec0)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_init_entries, dim3(static_cast<uint32_t>((n + 255u) / 256u)), dim3(256), 0, s,
                       d_entries, n, base, stride, rec0);
    return hipGetLastError();
}
