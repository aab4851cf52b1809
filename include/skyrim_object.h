/* C ABI of weather objects on the device: the contiguous regions where a field of M member states is beyond a threshold, labelled,
 * numbered and measured where the states lie in HBM.  Label and id planes stay on the device; 128-byte records and an int32 count
 * plane per request plane go back to the caller, which turns them into areas, centroids, axes and probabilities
 * (skyrim_amd/objects.py).
 *
 * Conventions of skyrim_track.h: all data pointers are device pointers; every call is asynchronous on `stream` (a hipStream_t); nothing
 * is allocated inside; the return code is 0, SKOBJ_E_ARG or SKOBJ_E_HIP; argument errors are found before anything touches the GPU, so
 * they are reported on a machine without one.  The three calls share one descriptor and each reads the fields listed at its name.
 *
 * ---- definitions ---------------------------------------------------------------------------------------------------------------------
 * Inputs.  M member states (1 <= M <= SKOBJ_MAX_MEMBERS), contiguous float32 (C, H, W), through a DEVICE array of M member pointers;
 * rows j, columns i, point index q = j W + i.  P planes (1 <= P <= SKOBJ_MAX_PLANES), each {channel, threshold, direction (+1: >=,
 * -1: <=), connectivity (4 or 8), value_scale}; one `periodic` flag for the grid; min_pixels >= 1; capacity >= 1 objects kept per
 * member and plane.  Plane arrays are indexed [m][p][j][i].
 *
 * Mask.  v >= thr (direction +1) or v <= thr (direction -1) in fp32; a NaN is background.
 *
 * Neighbourhood.  4-connectivity joins (j, i) to (j, i +- 1) and (j +- 1, i); 8-connectivity adds the four diagonals.  With `periodic`
 * (a global longitude circle) column W - 1 neighbours column 0, including the diagonals under 8-connectivity; without it (a regional
 * box) it does not.  Rows are NOT joined across the poles: row 0 and row H - 1 have no neighbours beyond them, so an object that
 * covers a pole on the sphere is one object only if its points in the pole row are joined along that row.
 *
 * Label.  L[q] = 1 + min{r : r in the component of q}, 0 on background.  The label depends on the mask alone, not on the order of
 * execution: the label plane is bitwise reproducible and equals a host flood fill.
 *
 * Objects.  The components of at least min_pixels points, numbered 1 .. n in ascending order of their smallest index.  Id plane:
 * I[q] = the object's number; 0 on background, on a component below min_pixels and on an object numbered above `capacity`.
 * n_found[m][p] = n counts every qualifying component, also beyond `capacity` (the convention of sktrack_detect: the counter keeps
 * counting and nothing else is touched).
 *
 * Record.  skobj_record, 128 bytes, one per kept object, at records[(m P + p) capacity + id - 1]; the slots of ids above
 * min(n, capacity) are not touched.  All accumulation is integer (atomic adds on 64-bit integers, integer atomic min / max): there is
 * no floating-point atomic anywhere, so every field is independent of the order of arrival.
 *   member, plane, id     where the record belongs
 *   root                  the object's smallest point index (its label minus 1)
 *   n_pixels, jmin, jmax  its points and its first and last row
 *   saturated             the points whose value was clamped in sum_v (below)
 *   area, sx .. szz       sums over the object's points of integers made from host tables (float64, scaled by 2^52).  With a_j the
 *                         fraction of the sphere's area of one cell of row j, phi the latitude and lambda the longitude:
 *                           row_tables[6][H]: a_j, a_j cos phi, a_j sin phi, a_j cos^2 phi, a_j cos phi sin phi, a_j sin^2 phi  (x 2^52)
 *                           col_tables[5][W]: cos lambda, sin lambda, cos^2 lambda, cos lambda sin lambda, sin^2 lambda
 *                         and, with R_k = row_tables[k][j], C_k = col_tables[k][i], rn = round to nearest integer, ties to even
 *                         (llrint), and every product ONE IEEE double multiplication:
 *                           area = sum rn(R_0)       sx  = sum rn(R_1 C_0)   sy  = sum rn(R_1 C_1)   sz  = sum rn(R_2)
 *                           sxx  = sum rn(R_3 C_2)   sxy = sum rn(R_3 C_3)   sxz = sum rn(R_4 C_0)
 *                           syy  = sum rn(R_3 C_4)   syz = sum rn(R_4 C_1)   szz = sum rn(R_5)
 *                         (x, y, z) = (cos phi cos lambda, cos phi sin lambda, sin phi) is the unit vector of the point.  A numpy
 *                         restatement with np.rint gives the same integers.  The a_j of a grid sum to at most 1, |R_k| <= R_0 and
 *                         |C_k| <= 1, so every sum stays below 2^53 in magnitude and the host reads it into a double exactly.
 *   sum_v                 sum rn(x A_j), x = clamp((double)v / value_scale, -4096, +4096), A_j = rn(R_0) 2^-12 (exact: a_j 2^40).
 *                         value_scale is a positive power of two chosen by the host (the power of two at or above |thr|, 1 for
 *                         thr = 0), so the division is exact; a point with |v / value_scale| > 4096 counts in `saturated`.
 *                         |x A_j| <= 2^12 a_j 2^40: the sum stays below 2^53 as well.
 *   ext_value, ext_index  the most extreme value in the plane's direction (the largest for >=, the smallest for <=) and its point
 *                         index; ties go to the lower index.  Made with one integer atomic max on the 64-bit key
 *                           (o << 32) | (0xffffffff - q),  k = the bits of v,  o' = k ^ (k >> 31 ? 0xffffffff : 0x80000000),
 *                           o = o' for >=, ~o' for <=
 *                         o' orders floats as the reals are ordered, with -0 below +0: a tie is a tie of bits.
 *
 * Bound on the mean.  The host takes the area-weighted mean as  value_scale sum_v / (area 2^-12).  With no point saturated, exact
 * arithmetic on the same inputs gives  value_scale (sum x A_j) / (sum A_j); area 2^-12 = sum A_j exactly, and each of the n_pixels
 * terms of sum_v is within 0.5 of x A_j, so
 *   |mean - exact| <= 0.5 n_pixels value_scale / (area 2^-12) = 0.5 n_pixels 2^-40 value_scale / area_fraction,
 * area_fraction = area 2^-52 being the object's share of the sphere.
 *
 * Probability.  keep[M][P][capacity + 1] (uint8, made by the host from the records; entry 0 of every row is 0) and the id planes give
 * count[p][j][i] = sum over m of keep[m][p][I[m][p][j][i]] (int32); the host divides by M.
 *
 * ---- shape of the computation --------------------------------------------------------------------------------------------------------
 * skobj_label: (1) a workgroup masks and labels one tile of 16 rows x 64 columns in LDS -- union by atomicMin on parent indices, each
 * point with its W, N and, under 8-connectivity, NW and NE neighbours -- and writes each point's parent as a global index; (2) the
 * points of the first row and of the first and last column of every tile are joined to their neighbours in the next tile, the wrap
 * column included, by the same union in global memory; (3) a flatten pass makes every label the root's and counts the points per root
 * (one integer add per wave where the wave's points share a root); (4) the qualifying roots are counted per chunk of 1024 points,
 * (5) the chunk counts are scanned per plane, which also gives n_found, (6) the roots are numbered in raster order and (7) the id
 * plane is written.  skobj_attributes: the kept records are initialised, one wave per (plane, row) walks the row and sums its
 * points in registers while they share an id, reducing over the wave before the atomics (integers: no bit changes), and a last pass
 * turns the extreme's key into ext_value and ext_index and reads `root` from the label plane.  skobj_probability: a streaming gather.
 * Kernel boundaries on the stream are the only phase boundaries: no workgroup ever waits for another.
 *
 * Limits: C H W <= 2^30; member pointers 4-byte aligned; labels, ids, n_found, counts 4-byte, tables, records and the workspace 8-byte
 * aligned; skobj_workspace_bytes(M, P, H, W) = 4 M P (H W + ceil(H W / 1024)) rounded up to 8; capacity <= 2^20. */
#ifndef SKYRIM_OBJECT_H
#define SKYRIM_OBJECT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SKOBJ_ABI_VERSION 1
#define SKOBJ_E_ARG (-1) /* bad argument: NULL or misaligned pointer, a count or index outside its range, a workspace too small */
#define SKOBJ_E_HIP (-2) /* a launch failed */
#define SKOBJ_MAX_MEMBERS 64
#define SKOBJ_MAX_PLANES 8
#define SKOBJ_CLAMP 4096.0 /* |v / value_scale| beyond this is clamped in sum_v and counted in `saturated` */

typedef struct {
    int32_t channel;
    float threshold;
    int32_t direction;    /* +1: v >= threshold, -1: v <= threshold */
    int32_t connectivity; /* 4 or 8 */
    float value_scale;    /* a positive power of two */
    int32_t pad;
} skobj_plane;

typedef struct {
    int32_t member, plane, id, root, n_pixels, jmin, jmax, saturated;
    int64_t area, sx, sy, sz, sxx, sxy, sxz, syy, syz, szz, sum_v;
    float ext_value;
    int32_t ext_index;
} skobj_record;

typedef struct {
    const float* const* members; /* device array of M device pointers                             label, attributes */
    int M;
    int C, H, W;
    int P;
    skobj_plane planes[SKOBJ_MAX_PLANES];
    int periodic;                /* 1: column W - 1 neighbours column 0                            label */
    int min_pixels;              /*                                                               label */
    int capacity;                /* objects kept per member and plane                             all three */
    int32_t* labels;             /* [M][P][H][W]: written by label, read by attributes */
    int32_t* ids;                /* [M][P][H][W]: written by label, read by attributes and probability */
    int32_t* n_found;            /* [M][P]: written by label, read by attributes */
    void* workspace;             /*                                                               label */
    size_t workspace_bytes;
    const double* row_tables;    /* [6][H]                                                        attributes */
    const double* col_tables;    /* [5][W]                                                        attributes */
    skobj_record* records;       /* [M][P][capacity]                                              attributes */
    const uint8_t* keep;         /* [M][P][capacity + 1]                                          probability */
    int32_t* counts;             /* [P][H][W]                                                     probability */
} skobj_desc;

int skobj_abi_version(void);

/* bytes of workspace skobj_label needs; 0 for arguments it would refuse */
size_t skobj_workspace_bytes(int M, int P, int H, int W);

int skobj_label(const skobj_desc* desc, void* stream);
int skobj_attributes(const skobj_desc* desc, void* stream);
int skobj_probability(const skobj_desc* desc, void* stream);

#ifdef __cplusplus
}
#endif
#endif
