// qc.hip -- quality control and sample selection on the 2-bit matrix: per-column genotype counts and per-row missing counts
// under row / column masks (mih_snp_counts), and a new matrix made of a selection of rows and columns of another
// (mih_snp_subset).  Replaces the SnpArrays.filter / SnpArrays.maf calls and the sample selection that open the reference's
// analysis pipelines (manuscript/NFBC_sim/NFBC_data_qc.jl, manuscript/UKBB_metabolomic/data_process.jl; src/utilities.jl:687-693).
#include "common.h"
#include <algorithm>

namespace mih {

constexpr int kQcBpPerBlock = 64;          // block pairs (128 rows) one workgroup of four waves walks
constexpr int kQcListRows = 8192;          // rows whose missing counts one workgroup of k_missing_counts keeps in LDS
constexpr int kQcListCols = 256;           // ... and the columns whose lists it visits

// dword index of the 16 rows 16 t .. 16 t + 15 inside a column's lane records, relative to the record (bp = 0, h = 0) of the
// column: t = 8 bp + 4 e + 2 h + u lives in dword 2 e + u of lane half h of block pair bp
__device__ __forceinline__ int64_t dword_of(int64_t t)
{
    return (t >> 3) * 256 + ((t >> 1) & 1) * 128 + ((t >> 2) & 1) * 2 + (t & 1);
}

// ---- masked counts -------------------------------------------------------------------------------------------------------------
// The row mask in the tiles' own row order: mask[(2 bp + h) * 4 + (2 e + u)] has both bits of row s set where row
// 128 bp + 64 e + 32 h + 16 u + s is kept (keep == nullptr: where it is a row of the matrix), so that a lane ANDs its record
// with one 16-byte word that all 32 columns of the tile share.
__global__ void k_expand_row_mask(const uint8_t *__restrict__ keep, int64_t n, int64_t nbp, uint32_t *__restrict__ mask)
{
    const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (t >= nbp * 8) return;
    uint32_t m = 0;
    for (int s = 0; s < 16; ++s) {
        const int64_t i = t * 16 + s;
        if (i < n && (!keep || keep[i])) m |= 3u << (2 * s);
    }
    mask[((t >> 3) * 2 + ((t >> 1) & 1)) * 4 + ((t >> 2) & 1) * 2 + (t & 1)] = m;
}

// n1 and n2 of every kept column over the kept rows: cnt[4 j + 1], cnt[4 j + 2].  Workgroup b walks block pairs
// [64 (b % nchunk), +64) of column group b / nchunk, a wave one tile per trip (one coalesced 1 KB load); a group without a kept
// column is not read.
__global__ void __launch_bounds__(256)
k_masked_counts(const uint4 *__restrict__ X, int64_t nbp, int64_t p, int64_t nchunk, const uint4 *__restrict__ mask,
                const uint8_t *__restrict__ col_keep, int32_t *__restrict__ cnt)
{
    __shared__ int32_t red[2][32];
    __shared__ int any;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = lane & 31, h = lane >> 5;
    const int64_t cg = blockIdx.x / nchunk, bp0 = (blockIdx.x % nchunk) * kQcBpPerBlock;
    const int64_t j = cg * 32 + m;
    const bool live = j < p && (!col_keep || col_keep[j]);
    if (threadIdx.x == 0) any = 0;
    if (threadIdx.x < 64) red[threadIdx.x >> 5][threadIdx.x & 31] = 0;
    __syncthreads();
    if (live && threadIdx.x < 32) atomicOr(&any, 1);
    __syncthreads();
    if (!any) return;
    int32_t c1 = 0, c2 = 0;
    for (int64_t bp = bp0 + w; bp < bp0 + kQcBpPerBlock && bp < nbp; bp += 4) {
        const uint4 v = X[(cg * nbp + bp) * 64 + lane], k = mask[bp * 2 + h];
        c1 += __popc(v.x & 0x55555555u & k.x) + __popc(v.y & 0x55555555u & k.y) + __popc(v.z & 0x55555555u & k.z) + __popc(v.w & 0x55555555u & k.w);
        c2 += __popc(v.x & 0xAAAAAAAAu & k.x) + __popc(v.y & 0xAAAAAAAAu & k.y) + __popc(v.z & 0xAAAAAAAAu & k.z) + __popc(v.w & 0xAAAAAAAAu & k.w);
    }
    if (live) { atomicAdd(&red[0][m], c1); atomicAdd(&red[1][m], c2); }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int k = threadIdx.x >> 5, mm = threadIdx.x & 31;
        if (red[k][mm]) atomicAdd(&cnt[4 * (cg * 32 + mm) + 1 + k], red[k][mm]);       // (only kept columns have added)
    }
}

// The missing entries of the kept columns in the kept rows, from the lists alone: cnt[4 j + 3] per column and row_missing[i]
// per row (nullptr: not asked for).  grid (chunks of 8192 rows, chunks of 256 columns), eight waves: the chunk's part of the row
// mask goes to LDS; one thread per column finds by bisection where the column's list (ascending rows) enters and leaves the
// chunk -- all columns at once, the walk is latency and nothing else; then a wave takes a column at a time, two entries per
// lane and trip.  The rows' counts gather in LDS and leave as one atomic per row that has any.
__global__ void __launch_bounds__(512)
k_missing_counts(const int64_t *__restrict__ miss_ptr, const int32_t *__restrict__ miss_row, int64_t n, int64_t p,
                 const uint8_t *__restrict__ row_keep, const uint8_t *__restrict__ col_keep, int32_t *__restrict__ cnt,
                 int32_t *__restrict__ row_missing)
{
    __shared__ int32_t rm[kQcListRows];
    __shared__ uint8_t keep[kQcListRows];
    __shared__ int64_t lo[kQcListCols], hi[kQcListCols];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kQcListRows, r1 = min(r0 + (int64_t)kQcListRows, n);
    const int64_t j0 = (int64_t)blockIdx.y * kQcListCols, j1 = min(j0 + (int64_t)kQcListCols, p);
    for (int i = threadIdx.x; i < kQcListRows; i += 512) {
        rm[i] = 0;
        keep[i] = r0 + i < r1 && (!row_keep || row_keep[r0 + i]);
    }
    if (threadIdx.x < kQcListCols) {
        const int64_t j = j0 + threadIdx.x;
        int64_t a = 0, e = 0;
        if (j < j1 && (!col_keep || col_keep[j])) {
            a = miss_ptr[j];
            const int64_t b = miss_ptr[j + 1];
            for (int64_t top = b; a < top;) {                    // the first entry with row >= r0
                const int64_t mid = a + ((top - a) >> 1);
                if ((int64_t)miss_row[mid] < r0) a = mid + 1; else top = mid;
            }
            e = a;
            for (int64_t top = b; e < top;) {                    // ... and the first with row >= r1
                const int64_t mid = e + ((top - e) >> 1);
                if ((int64_t)miss_row[mid] < r1) e = mid + 1; else top = mid;
            }
        }
        lo[threadIdx.x] = a; hi[threadIdx.x] = e;
    }
    __syncthreads();
    for (int c = w; c < (int)(j1 - j0); c += 8) {               // (the same trips and bounds for every lane of a wave)
        const int64_t a = lo[c], e = hi[c];
        int32_t k = 0;
        for (int64_t t0 = a; t0 < e; t0 += 128) {
            const int64_t t1 = t0 + lane, t2 = t1 + 64;
            const int32_t i1 = t1 < e ? (int32_t)(miss_row[t1] - r0) : -1, i2 = t2 < e ? (int32_t)(miss_row[t2] - r0) : -1;
            const bool h1 = i1 >= 0 && keep[i1], h2 = i2 >= 0 && keep[i2];
            if (row_missing) {
                if (h1) atomicAdd(&rm[i1], 1);
                if (h2) atomicAdd(&rm[i2], 1);
            }
            k += __popcll(__ballot(h1)) + __popcll(__ballot(h2));
        }
        if (lane == 0 && k) atomicAdd(&cnt[4 * (j0 + c) + 3], k);
    }
    if (row_missing) {
        __syncthreads();
        for (int i = threadIdx.x; i < kQcListRows; i += 512)
            if (rm[i]) atomicAdd(&row_missing[r0 + i], rm[i]);
    }
}

// ---- subset --------------------------------------------------------------------------------------------------------------------
// The lane records of the result.  Result column j' is source column cols[j'] (nullptr: j').  The rows come as a recipe that
// all columns share: the 16 rows of result dword t are the runs run[roff[t]] .. run[roff[t + 1]), a run being consecutive kept
// source rows inside one source dword -- .x the source dword (row / 16), .y = its first row's place there | the place of the
// run in the result dword << 4 | its length << 8 -- so a result dword costs a shift and a mask per run, not per row: three
// runs or so where a few rows in a hundred are dropped, sixteen where the selection is sparse (roff == nullptr: every row, a
// plain copy of the column's dwords).  Workgroup b builds block pairs [64 (b % nchunk), +64) of result column group b / nchunk,
// a wave one tile per trip: lane 32 h + m gathers the four dwords of column m, dword 2 e + u the result rows
// 128 bp + 64 e + 32 h + 16 u + (0..15), loading a source dword once however many runs it holds.  The runs are the same for the
// 32 columns of a half wave, so its lanes load together, 512 contiguous bytes where the columns are neighbours, and the span
// of source tiles behind a result tile is whatever the selection makes it: nothing is staged.  The source has its missing
// entries as code 0 and so has the result: its lists come from the source's (k_kept_missing).  Every record of every tile is
// written, the pad columns' and pad rows' as zeros; n1 and n2 are counted into cnt[3 j' + {0, 1}].
__global__ void __launch_bounds__(256)
k_subset_tiles(const uint32_t *__restrict__ S, int64_t s_nbp, const int32_t *__restrict__ roff, const int2 *__restrict__ run,
               const int64_t *__restrict__ cols, int64_t n_out, int64_t p_out, uint4 *__restrict__ X, int64_t nbp, int64_t nchunk,
               int32_t *__restrict__ cnt)
{
    __shared__ int32_t red[2][32];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, m = lane & 31, h = lane >> 5;
    const int64_t cg = blockIdx.x / nchunk, bp0 = (blockIdx.x % nchunk) * kQcBpPerBlock;
    const int64_t j = cg * 32 + m;
    const bool live = j < p_out;
    const int64_t js = live ? (cols ? cols[j] : j) : 0;
    const uint32_t *col = S + (((js >> 5) * s_nbp * 64 + (js & 31)) << 2);
    if (threadIdx.x < 64) red[threadIdx.x >> 5][threadIdx.x & 31] = 0;
    __syncthreads();
    int32_t c1 = 0, c2 = 0;
    for (int64_t bp = bp0 + w; bp < bp0 + kQcBpPerBlock && bp < nbp; bp += 4) {
        uint32_t d[4] = {0u, 0u, 0u, 0u};
        #pragma unroll
        for (int q = 0; q < 4; ++q) {                            // q = 2 e + u
            const int64_t t = bp * 8 + (q >> 1) * 4 + h * 2 + (q & 1);
            if (!live || t * 16 >= n_out) continue;
            uint32_t out = 0;
            if (roff) {
                int32_t have = -1;
                uint32_t word = 0;
                for (int32_t k = roff[t], k1 = roff[t + 1]; k < k1; ++k) {
                    const int2 r = run[k];
                    if (r.x != have) { word = col[dword_of(r.x)]; have = r.x; }
                    out |= ((word >> (2 * (r.y & 15))) & (0xFFFFFFFFu >> (32 - 2 * (r.y >> 8)))) << (2 * ((r.y >> 4) & 15));
                }
            } else {
                out = col[dword_of(t)];                          // (rows >= n are zeros in the source too)
            }
            d[q] = out;
            c1 += __popc(out & 0x55555555u);
            c2 += __popc(out & 0xAAAAAAAAu);
        }
        X[(cg * nbp + bp) * 64 + lane] = make_uint4(d[0], d[1], d[2], d[3]);
    }
    if (live) { atomicAdd(&red[0][m], c1); atomicAdd(&red[1][m], c2); }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int k = threadIdx.x >> 5, mm = threadIdx.x & 31;
        if (red[k][mm]) atomicAdd(&cnt[3 * (cg * 32 + mm) + k], red[k][mm]);
    }
}

// One wave per result column over the source column's missing list (ascending rows): the entries whose rows are kept --
// inv[i] is the result row of source row i, -1 if it is dropped (nullptr: i itself) -- are counted into cnt[3 j' + 2]
// (out == nullptr), or written as result rows to out[ptr[j'] ..] in the same, still ascending, order.
__global__ void __launch_bounds__(64)
k_kept_missing(const int64_t *__restrict__ s_ptr, const int32_t *__restrict__ s_row, const int32_t *__restrict__ inv,
               const int64_t *__restrict__ cols, int32_t *__restrict__ cnt, const int64_t *__restrict__ ptr, int32_t *__restrict__ out)
{
    const int lane = threadIdx.x;
    const int64_t j = blockIdx.x, js = cols ? cols[j] : j;
    const int64_t a = s_ptr[js], b = s_ptr[js + 1];
    const int64_t base = out ? ptr[j] : 0;
    int32_t c = 0;
    for (int64_t t0 = a; t0 < b; t0 += 64) {
        const int64_t t = t0 + lane;
        int32_t i = -1;
        if (t < b) { const int32_t is = s_row[t]; i = inv ? inv[is] : is; }
        const unsigned long long kept = __ballot(i >= 0);
        if (out && i >= 0) out[base + c + __popcll(kept & ((1ull << lane) - 1ull))] = i;
        c += __popcll(kept);
    }
    if (!out && lane == 0) cnt[3 * j + 2] = c;
}

void launch_missing_counts(const mih_mat *h, const uint8_t *row_keep_dev, const uint8_t *col_keep_dev, int32_t *cnt4,
                           int32_t *row_missing, hipStream_t s)
{
    const int64_t n = h->n, p = h->p;
    const int64_t slab = 65535ll * kQcListCols;                  // (grid.y stays below 65536)
    for (int64_t c0 = 0; c0 < p; c0 += slab) {
        const int64_t nc = std::min(slab, p - c0);
        dim3 grid((unsigned)((n + kQcListRows - 1) / kQcListRows), (unsigned)((nc + kQcListCols - 1) / kQcListCols));
        hipLaunchKernelGGL(k_missing_counts, grid, dim3(512), 0, s, h->miss_ptr + c0, h->miss_row, n, nc, row_keep_dev,
                           col_keep_dev ? col_keep_dev + c0 : nullptr, cnt4 + 4 * c0, row_missing);
    }
}

// a selection (strictly increasing 0-based indices below `len`, or nullptr for everything): how many, or -1 with the error set
static int64_t check_selection(const char *what, const int64_t *idx, int64_t count, int64_t len)
{
    if (!idx) return len;
    if (count <= 0) { set_error("the selection of %s is empty", what); return -1; }
    for (int64_t t = 0; t < count; ++t) {
        if (idx[t] < 0 || idx[t] >= len) {
            set_error("%s index %lld (entry %lld of the selection) is outside 0 .. %lld", what, (long long)idx[t], (long long)t, (long long)(len - 1));
            return -1;
        }
        if (t > 0 && idx[t] <= idx[t - 1]) {
            set_error("the %s indices must be strictly increasing: entry %lld is %lld after %lld", what, (long long)t, (long long)idx[t], (long long)idx[t - 1]);
            return -1;
        }
    }
    return count;
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_snp_counts(const mih_mat *h, const uint8_t *row_keep, const uint8_t *col_keep, int32_t *col_counts, int32_t *row_missing)
{
    if (!h || h->kind != 0) { set_error("mih_snp_counts needs a 2-bit (SnpLinAlg) handle"); return MIH_BAD_ARG; }
    if (!col_counts && !row_missing) return MIH_OK;
    const int64_t n = h->n, p = h->p;
    MIH_HIP(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    DevBuf<uint8_t> rk, ck;
    DevBuf<int32_t> cnt, rm;
    DevBuf<uint32_t> mask;
    int64_t kept_rows = n;
    if (row_keep) {
        kept_rows = 0;
        for (int64_t i = 0; i < n; ++i) kept_rows += row_keep[i] != 0;
        MIH_TRY(rk.alloc((size_t)n));
        MIH_HIP(hipMemcpyAsync(rk.p, row_keep, (size_t)n, hipMemcpyHostToDevice, s));
    }
    if (col_keep) {
        MIH_TRY(ck.alloc((size_t)p));
        MIH_HIP(hipMemcpyAsync(ck.p, col_keep, (size_t)p, hipMemcpyHostToDevice, s));
    }
    MIH_TRY(cnt.alloc((size_t)(4 * p)));
    MIH_HIP(hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * 4 * (size_t)p, s));
    if (row_missing) {
        MIH_TRY(rm.alloc((size_t)n));
        MIH_HIP(hipMemsetAsync(rm.p, 0, sizeof(int32_t) * (size_t)n, s));
    }
    if (col_counts) {                                            // the one pass over the tiles
        const int64_t nchunk = (h->nbp + kQcBpPerBlock - 1) / kQcBpPerBlock;
        if (h->ncg * nchunk >= (1ll << 31)) { set_error("the matrix has too many tiles for one launch"); return MIH_BAD_DIM; }
        MIH_TRY(mask.alloc((size_t)h->nbp * 8));
        hipLaunchKernelGGL(k_expand_row_mask, dim3((unsigned)((h->nbp * 8 + 255) / 256)), dim3(256), 0, s, rk.p, n, h->nbp, mask.p);
        hipLaunchKernelGGL(k_masked_counts, dim3((unsigned)(h->ncg * nchunk)), dim3(256), 0, s, reinterpret_cast<const uint4 *>(h->X), h->nbp, p,
                           nchunk, reinterpret_cast<const uint4 *>(mask.p), ck.p, cnt.p);
    }
    if (h->total_missing > 0) launch_missing_counts(h, rk.p, ck.p, cnt.p, rm.p, s);
    if (col_counts) MIH_HIP(hipMemcpyAsync(col_counts, cnt.p, sizeof(int32_t) * 4 * (size_t)p, hipMemcpyDeviceToHost, s));
    if (row_missing) MIH_HIP(hipMemcpyAsync(row_missing, rm.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    MIH_HIP(hipStreamSynchronize(s));
    if (col_counts)                                              // missing entries and pad rows are code 0 in the tiles: n0 is what is left
        for (int64_t j = 0; j < p; ++j)
            if (!col_keep || col_keep[j]) col_counts[4 * j] = (int32_t)(kept_rows - col_counts[4 * j + 1] - col_counts[4 * j + 2] - col_counts[4 * j + 3]);
    return MIH_OK;
}

int mih_snp_subset(const mih_mat *src, const int64_t *rows, int64_t nrows, const int64_t *cols, int64_t ncols,
                   int center, int scale, int impute, int dtype, mih_mat **out)
{
    if (!out) { set_error("null argument"); return MIH_BAD_ARG; }
    *out = nullptr;
    if (!src || src->kind != 0) { set_error("mih_snp_subset needs a 2-bit (SnpLinAlg) handle"); return MIH_BAD_ARG; }
    if (dtype != 64 && dtype != 32) { set_error("dtype must be 64 (SnpLinAlg{Float64}) or 32 (SnpLinAlg{Float32})"); return MIH_BAD_ARG; }
    const int64_t n = check_selection("row", rows, nrows, src->n);
    if (n < 0) return MIH_BAD_ARG;
    const int64_t p = check_selection("column", cols, ncols, src->p);
    if (p < 0) return MIH_BAD_ARG;
    MIH_HIP(hipSetDevice(src->device));

    // the rows' recipe (k_subset_tiles) and the inverse row map, O(n) each; the column list, O(p)
    DevBuf<int32_t> roff, inv, cnt;
    DevBuf<int2> run;
    DevBuf<int64_t> cmap;
    if (rows) {
        const int64_t ndw = (n + 15) / 16;
        std::vector<int32_t> hoff((size_t)ndw + 1, 0), hinv((size_t)src->n, -1);
        std::vector<int2> hrun;
        hrun.reserve((size_t)ndw * 3);
        for (int64_t t = 0; t < ndw; ++t) {
            const int64_t end = std::min(n, 16 * t + 16);
            for (int64_t i = 16 * t; i < end;) {
                const int64_t r = rows[i];
                int64_t len = 1;
                while (i + len < end && rows[i + len] == r + len && ((r + len) & 15) != 0) ++len;
                hrun.push_back(make_int2((int)(r >> 4), (int)((r & 15) | ((i & 15) << 4) | (len << 8))));
                i += len;
            }
            hoff[(size_t)t + 1] = (int32_t)hrun.size();
        }
        for (int64_t i = 0; i < n; ++i) hinv[(size_t)rows[i]] = (int32_t)i;
        MIH_TRY(roff.alloc(hoff.size()));
        MIH_TRY(run.alloc(hrun.size()));
        MIH_TRY(inv.alloc(hinv.size()));
        MIH_HIP(hipMemcpy(roff.p, hoff.data(), sizeof(int32_t) * hoff.size(), hipMemcpyHostToDevice));
        MIH_HIP(hipMemcpy(run.p, hrun.data(), sizeof(int2) * hrun.size(), hipMemcpyHostToDevice));
        MIH_HIP(hipMemcpy(inv.p, hinv.data(), sizeof(int32_t) * hinv.size(), hipMemcpyHostToDevice));
    }
    if (cols) {
        MIH_TRY(cmap.alloc((size_t)p));
        MIH_HIP(hipMemcpy(cmap.p, cols, sizeof(int64_t) * (size_t)p, hipMemcpyHostToDevice));
    }
    MIH_TRY(cnt.alloc((size_t)(3 * p)));

    mih_mat *h = new mih_mat();
    h->kind = 0; h->device = src->device; h->n = n; h->p = p;
    h->center = center; h->scale = scale; h->impute = impute;
    auto fail = [&](int code) { mih_mat_destroy(h); return code; };
    int rc = alloc_snp(h);
    if (rc) return fail(rc);
    if (hipStreamCreate(&h->stream) != hipSuccess) return fail(MIH_HIP_ERROR);
    const int64_t nchunk = (h->nbp + kQcBpPerBlock - 1) / kQcBpPerBlock;
    if (h->ncg * nchunk >= (1ll << 31)) { set_error("the selection has too many tiles for one launch"); return fail(MIH_BAD_DIM); }
    if (hipStreamSynchronize(src->stream) != hipSuccess) return fail(MIH_HIP_ERROR);      // whatever was queued on the source has finished
    if (hipMemsetAsync(cnt.p, 0, sizeof(int32_t) * 3 * (size_t)p, h->stream) != hipSuccess) return fail(MIH_HIP_ERROR);
    hipLaunchKernelGGL(k_subset_tiles, dim3((unsigned)(h->ncg * nchunk)), dim3(256), 0, h->stream, src->X, src->nbp, roff.p, run.p, cmap.p, n, p,
                       reinterpret_cast<uint4 *>(h->X), h->nbp, nchunk, cnt.p);
    if (src->total_missing > 0)
        hipLaunchKernelGGL(k_kept_missing, dim3((unsigned)p), dim3(64), 0, h->stream, src->miss_ptr, src->miss_row, inv.p, cmap.p, cnt.p,
                           (const int64_t *)nullptr, (int32_t *)nullptr);
    if ((rc = finish_counts(h, cnt.p))) return fail(rc);        // mu, sinv and the lists' offsets, as after a transcode
    if (h->total_missing > 0)
        hipLaunchKernelGGL(k_kept_missing, dim3((unsigned)p), dim3(64), 0, h->stream, src->miss_ptr, src->miss_row, inv.p, cmap.p, cnt.p,
                           h->miss_ptr, h->miss_row);
    if (hipStreamSynchronize(h->stream) != hipSuccess) {
        set_error("the subset kernels failed: %s", hipGetErrorString(hipGetLastError()));
        return fail(MIH_HIP_ERROR);
    }
    reserve_fit_memory(h);
    *out = h;
    return MIH_OK;
}

}  // extern "C"
