/* C ABI of packed member archives on the device: the listed channels of M member states are quantised plane by plane to 16-bit codes in
 * the byte order of a netCDF-3 file (skpack_range, then skpack_quantize), and a packed state is turned back into float32 (skpack_unpack).
 * It is the ensemble's counterpart of skio_bswap32: what crosses PCIe and lands on disk is half of the float32 state, and the host only
 * calls pwrite.
 *
 * Conventions of skyrim_point.h and skyrim_clim.h: all data pointers are device pointers; every call is asynchronous on `stream` (a
 * hipStream_t); nothing is allocated inside; the return code is 0, SKPACK_E_ARG or SKPACK_E_HIP; argument errors are found before anything
 * touches the GPU, so they are reported on a machine without one.  Every operation is rounded on its own: the library is built with
 * contraction to fma OFF (-ffp-contract=off).  fp32 subnormals are KEPT (hipcc's default mode): a subnormal input is a finite value like
 * any other, lo and hi may be subnormal, and no operation below flushes one to zero.  No atomics (integer or float), no scratch (no
 * register array is indexed at run time), LDS only for the reduction of a workgroup, 32-bit byte offsets inside a state.
 *
 * `members`: a DEVICE array of M pointers to contiguous float32 states (C, H, W), 1 <= M <= SKPACK_MAX_MEMBERS, each 4-byte aligned.
 * `channels`: a HOST list of nc channel indices, 1 <= nc <= SKPACK_MAX_CHANNELS, each in [0, C), any order, repeats allowed.  A PLANE is
 * the H W values of one listed channel of one member; plane (m, k) has the table record table[m nc + k].
 *
 * ---- skpack_range ---------------------------------------------------------------------------------------------------------------------
 * Per plane, over its FINITE values (|x| < inf): lo = the minimum, hi = the maximum, n_bad = the number of NaN and +-Inf.  Then, all on
 * the device (no host round trip between this call and skpack_quantize):
 *      lo = fl32(lo + 0.0f), hi = fl32(hi + 0.0f)                    so -0 is +0
 *      in IEEE double, every operation rounded on its own:
 *      offset = fl(fl(0.5 lo) + fl(0.5 hi))      d = fl(hi - lo)      scale = fl(d / 65534.0)      inv = fl(65534.0 / d)
 *      d == 0 (a constant plane):                scale = inv = 1
 *      no finite value:                          offset = 0, scale = inv = 1, lo = hi = 0
 * (0.5 lo and 0.5 hi are exact in double.  Their sum and hi - lo are exact where lo and hi have one sign and lie within 2^29 of each
 * other in magnitude; otherwise each carries one rounding, relative to a value no larger than d.)  pad = 0.  Minimum and maximum do not depend on the order of the comparisons and n_bad
 * is an integer sum, so the record is bitwise reproducible: a workgroup reduces a tile of SKPACK_RANGE_TILE consecutive values of a plane
 * to one partial (lo, hi, n_bad) in `workspace`, a second kernel reduces the partials of a plane and writes its record.  `workspace`: 4-byte
 * aligned, at least skpack_workspace_bytes(M, nc, H, W) = 12 M nc ceil(H W / SKPACK_RANGE_TILE) bytes; its contents need no preparation.
 *
 * ---- skpack_quantize ------------------------------------------------------------------------------------------------------------------
 * With the record t of the value's plane, in double:
 *      code = clamp(rint(fl(fl(double(x) - t.offset) t.inv)), -32767, 32767)          rint: to nearest, halves to even
 *      a non-finite x: code = -32768                                                  (the file's _FillValue)
 * The codes of member m are the flat (nc, H, W) array in C order, no padding between planes, as BIG-ENDIAN 16-bit integers from
 * out + m member_stride_bytes.  `out` is 2-byte aligned; member_stride_bytes is even and at least 2 nc H W.  NOTHING beyond the 2 nc H W
 * bytes of each member's part is written (gaps and tails keep their bytes).
 *
 * ---- skpack_unpack --------------------------------------------------------------------------------------------------------------------
 * One state: `codes` a device image of big-endian codes (nc, H, W) at any 2-byte alignment, `table` its nc records (only scale and offset
 * are read), `out` contiguous float32 (nc, H, W), 4-byte aligned:
 *      x' = fl32(fl(fl(double(code) t.scale) + t.offset))          code -32768: the quiet NaN 0x7FC00000
 *
 * ---- the bound ------------------------------------------------------------------------------------------------------------------------
 * For a finite x of a plane with record t, u = 2^-53:
 *      |x' - x| <= 0.5 t.scale (1 + 2^-20) + 2^-24 max(|t.lo|, |t.hi|) + 2^-149
 * Derivation.  Write m for the exact midpoint and s = d_exact / 65534.  offset, d and e = fl(double(x) - offset) carry one rounding each,
 * every one relative to a value of at most d (see above; x - offset is exact where x and offset are close, Sterbenz), so e = (x - m) +
 * g d with |g| <= 3 u.  q = fl(e inv) adds inv's rounding (d's and the division's) and the product's: q = (x - m) / s + h with |h| <=
 * 65534 (3 u + 1.6 u) < 2^-34.  rint moves q by at most 0.5, and the clamp only brings back a value that these roundings carried past
 * +-32767, so |code - (x - m) / s| <= 0.5 + 2^-34.  Decoding: t.scale is s (1 + 2 u), the product adds one rounding, the sum with offset one
 * more and offset's own: in double |x'' - x| <= A = 0.5 s (1 + 2^-32) + 2^-51 B with B = max(|lo|, |hi|).  The rounding of x'' to fp32 adds half
 * an ulp of x'', at most 2^-24 |x''| <= 2^-24 (B + A), or 2^-150 where the result is subnormal: |x' - x| <= A (1 + 2^-24) + 2^-24 B + 2^-150.
 * Where d >= 2^-13 B the 2^-51 B in A is below the 2^-21 s the stated bound adds to 0.5 s, and the bound holds.  Where d < 2^-13 B every
 * x of the plane has |x| >= B / 2 and neighbours at least 2^-25 B away, while A < 2^-30 B: x'' lies within a quarter of that of the fp32
 * number x and rounds to x itself, error 0.  (tests/test_pack_cpu.py checks both regimes numerically as well.)
 * Properties.  lo and hi get the codes -32767 and +32767: q = -+32767 + h with |h| < 2^-34 rounds to -+32767.  The codes of a constant
 * plane are all 0 (e = 0 exactly) and decode to fl32(0 1 + offset) = fl32(lo) = lo exactly.
 *
 * Shape of the computation.  All three are streaming passes with grid-stride over (member, channel, tile) units; the member pointer, the
 * plane's first element and the table record are wave-uniform (scalar loads).  A lane of skpack_quantize takes 8 consecutive values and
 * stores their 16 bytes at once where the OUTPUT address is 16-byte aligned: the few codes of a unit before the first and after the last
 * aligned address (a plane of odd size begins in the middle of a 32-bit word) are stored as single 16-bit values, so no store straddles
 * two planes or two table records.  Inputs are read as 16-byte vectors where the unit's first body value is 16-byte aligned, as single
 * values otherwise.  skpack_unpack mirrors it (16-byte loads of codes on the aligned body).  Bytes per element in HBM: range 4,
 * quantize 4 + 2, unpack 2 + 4.
 *
 * Limits: C H W <= 2^30 and nc H W <= 2^30, the pointer array 8-byte aligned, the table 8-byte aligned. */
#ifndef SKYRIM_PACK_H
#define SKYRIM_PACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKPACK_ABI_VERSION 1
#define SKPACK_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count, size, index or stride outside its range */
#define SKPACK_E_HIP (-2) /* a launch failed */
#define SKPACK_MAX_MEMBERS 1024
#define SKPACK_MAX_CHANNELS 256
#define SKPACK_RANGE_TILE 16384 /* values of a plane per partial of skpack_range */
#define SKPACK_FILL (-32768)    /* the code of a non-finite value */

typedef struct {
    double offset, scale, inv; /* x ~ code scale + offset; inv = 1 / scale as the header forms it */
    float lo, hi;              /* the finite range of the plane, -0 as +0 */
    int32_t n_bad;             /* NaN and +-Inf of the plane */
    int32_t pad;               /* 0 */
} skpack_entry;

typedef struct {
    const float* const* members; /* device array of M device pointers */
    int M;
    int C, H, W;                 /* the member states */
    int nc;                      /* listed channels */
    int32_t channels[SKPACK_MAX_CHANNELS];
    skpack_entry* table;         /* device, [M][nc]: written by skpack_range, read by skpack_quantize */
    void* workspace;             /* skpack_range: device, skpack_workspace_bytes(M, nc, H, W) at least; ignored by skpack_quantize */
    size_t workspace_bytes;
    void* out;                   /* skpack_quantize: device, the big-endian codes; ignored by skpack_range */
    size_t member_stride_bytes;  /* skpack_quantize: even, >= 2 nc H W */
} skpack_desc;

typedef struct {
    const void* codes;         /* device, big-endian int16 (nc, H, W), 2-byte aligned */
    const skpack_entry* table; /* device, nc records */
    int nc, H, W;
    float* out;                /* device, float32 (nc, H, W) */
} skpack_unpack_desc;

int skpack_abi_version(void);

/* bytes of workspace skpack_range needs; 0 for counts outside their ranges */
size_t skpack_workspace_bytes(int M, int nc, int H, int W);

int skpack_range(const skpack_desc* desc, void* stream);
int skpack_quantize(const skpack_desc* desc, void* stream);
int skpack_unpack(const skpack_unpack_desc* desc, void* stream);

/* the argument checks of the three calls alone: 0 or SKPACK_E_ARG for exactly the descriptors the calls take or refuse.  They touch no
 * GPU and read no device memory, so a caller (and a test on a machine without a GPU) can try a descriptor before its buffers exist */
int skpack_range_check(const skpack_desc* desc);
int skpack_quantize_check(const skpack_desc* desc);
int skpack_unpack_check(const skpack_unpack_desc* desc);

#ifdef __cplusplus
}
#endif
#endif
