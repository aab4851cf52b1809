// Point extraction (include/skyrim_point.h): one gather kernel over (tile of 256 points, chunk of listed channels, member).  A lane owns one
// point: it loads its record once, forms its four tap offsets once and walks the chunk's channels four at a time, the sixteen loads of a
// group issued before the first is used.  Contraction to fma is off for the whole file (and on the build line): the header fixes the order
// of the fp32 operations.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "../../include/skyrim_point.h"
#include "fields.h"

#pragma clang fp contract(off)

namespace {

constexpr int LANES = 256;       // of a workgroup: one tile of points
constexpr int CHUNK = SKPOINT_CHUNK;
constexpr int GROUP = 4;         // channels whose loads are in flight together

static_assert(sizeof(skpoint_rec) == 32, "a record is two 16-byte loads");
static_assert(CHUNK % GROUP == 0, "a chunk is whole groups");

struct PointArgs {
    int H, W, nc, P;
    size_t member_stride;
    uint32_t plane[SKPOINT_MAX_CHANNELS];       // first element of the k-th listed channel's plane: channels[k] H W
};

using namespace skfields;
typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(LANES) point_kernel(const PointArgs a, const float* const* __restrict__ members,
                                                       const skpoint_rec* __restrict__ records, float* __restrict__ out) {
    const uint32_t p = blockIdx.x * LANES + threadIdx.x;
    if (p >= (uint32_t)a.P) return;                                        // (no barrier below)
    const int k0 = blockIdx.y * CHUNK, k1 = min(k0 + CHUNK, a.nc);         // the chunk's listed channels; member and channel are uniform
    const uint32_t m = blockIdx.z;
    const float* x = members[m];
    const i32x4 ri = *(const SK_GLOBAL i32x4*)((const SK_GLOBAL char*)records + 32u * p);
    const f32x4 rw = *(const SK_GLOBAL f32x4*)((const SK_GLOBAL char*)records + 32u * p + 16u);
    // no access depends on the record beyond these clamps
    const int H = a.H, W = a.W;
    const int row = ri.x < 0 ? 0 : (ri.x > H - 1 ? H - 1 : ri.x);
    int col = ri.y % W;
    col = col < 0 ? col + W : col;
    const bool two_r = ri.z >= 2, two_c = ri.w >= 2;                       // counts clamped into [1, 2]
    // a tap that is not used aliases the first one: its load is valid and costs no further line, its value is dropped
    const int row1 = two_r ? min(row + 1, H - 1) : row;
    const int col1 = two_c ? (col + 1 == W ? 0 : col + 1) : col;
    const uint32_t o00 = (uint32_t)(row * W + col), o01 = (uint32_t)(row * W + col1);
    const uint32_t o10 = (uint32_t)(row1 * W + col), o11 = (uint32_t)(row1 * W + col1);
    const float wr0 = rw.x, wr1 = rw.y, wc0 = rw.z, wc1 = rw.w;
    float* y = out + (size_t)m * a.member_stride + p;
    for (int k = k0; k < k1; k += GROUP) {
        float x00[GROUP], x01[GROUP], x10[GROUP], x11[GROUP];
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {                                  // all loads of the group before the first use
            const uint32_t base = a.plane[min(k + g, k1 - 1)];             // (past the chunk's end: the last channel again, not stored)
            x00[g] = load_vec<1>(x, base + o00);
            x01[g] = load_vec<1>(x, base + o01);
            x10[g] = load_vec<1>(x, base + o10);
            x11[g] = load_vec<1>(x, base + o11);
        }
#pragma unroll
        for (int g = 0; g < GROUP; ++g) {
            float v0 = wr0 * x00[g], v1 = wr0 * x01[g];
            const float t0 = wr1 * x10[g], t1 = wr1 * x11[g];
            v0 = two_r ? v0 + t0 : v0;
            v1 = two_r ? v1 + t1 : v1;
            float r = wc0 * v0;
            const float t = wc1 * v1;
            r = two_c ? r + t : r;
            if (k + g < k1) y[(size_t)(k + g) * (size_t)a.P] = r;          // coalesced over p
        }
    }
}

// every refusal of skpoint_gather: nothing here touches the GPU
bool valid(const skpoint_desc* d) {
    if (!d || !d->members || ((uintptr_t)d->members & 7) || !d->out || ((uintptr_t)d->out & 3)) return false;
    if (!d->records || ((uintptr_t)d->records & 15)) return false;
    if (d->M < 1 || d->M > SKPOINT_MAX_MEMBERS || d->nc < 1 || d->nc > SKPOINT_MAX_CHANNELS) return false;
    if (d->P < 1 || d->P > SKPOINT_MAX_POINTS || d->C < 1 || d->H < 1 || d->W < 2) return false;
    const size_t lim = (size_t)1 << 30, HW = (size_t)d->H * (size_t)d->W;
    if (HW > lim || (size_t)d->C > lim / HW || (size_t)d->nc * (size_t)d->P > lim) return false;
    if (d->member_stride < (size_t)d->nc * (size_t)d->P) return false;
    for (int k = 0; k < d->nc; ++k)
        if (d->channels[k] < 0 || d->channels[k] >= d->C) return false;
    return true;
}

bool weight_ok(float w) { return std::isfinite(w) && w != 0.f; }

}  // namespace

extern "C" int skpoint_abi_version(void) { return SKPOINT_ABI_VERSION; }

extern "C" int skpoint_validate(const skpoint_rec* r, int P, int H, int W) {
    if (!r || P < 1 || H < 1 || W < 2) return SKPOINT_E_ARG;
    for (int p = 0; p < P; ++p) {
        const skpoint_rec& q = r[p];
        if (q.row < 0 || q.row >= H || q.col < 0 || q.col >= W) return SKPOINT_E_ARG;
        if ((q.nr != 1 && q.nr != 2) || (q.ncol != 1 && q.ncol != 2)) return SKPOINT_E_ARG;
        if (q.nr == 2 && q.row == H - 1) return SKPOINT_E_ARG;
        if (!weight_ok(q.wr0) || !weight_ok(q.wc0)) return SKPOINT_E_ARG;
        if ((q.nr == 2 && !weight_ok(q.wr1)) || (q.ncol == 2 && !weight_ok(q.wc1))) return SKPOINT_E_ARG;
    }
    return 0;
}

extern "C" int skpoint_gather(const skpoint_desc* d, void* stream) {
    if (!valid(d)) return SKPOINT_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    PointArgs a = {};
    a.H = d->H; a.W = d->W; a.nc = d->nc; a.P = d->P;
    a.member_stride = d->member_stride;
    for (int k = 0; k < d->nc; ++k) a.plane[k] = (uint32_t)d->channels[k] * (uint32_t)d->H * (uint32_t)d->W;
    const dim3 grid((unsigned)((d->P + LANES - 1) / LANES), (unsigned)((d->nc + CHUNK - 1) / CHUNK), (unsigned)d->M);
    hipLaunchKernelGGL(point_kernel, grid, dim3(LANES), 0, s, a, d->members, d->records, d->out);
    return hipGetLastError() == hipSuccess ? 0 : SKPOINT_E_HIP;
}
