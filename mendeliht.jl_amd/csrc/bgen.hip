// bgen.hip -- BGEN v1.2 genotype blocks streamed from disk into the 16-bit dosage matrix (mih_dosage_create_bgen).
//
// The caller walks the variant headers (genotypes.py: bgen_index) and hands over the file offset of each genotype block.  Host
// threads only read and inflate; the GPU unpacks.  T workers, each with its own stream, two pinned staging buffers and two device
// buffers (the scheme of the .bed ingest, snp.hip), take runs of consecutive blocks from one queue: pread the run, check each
// block header on the host and inflate it into the pinned buffer, DMA, and decode on the worker's stream (k_bgen_decode: one
// workgroup per chunk of 8192 samples of a block: k_bgen_scan, k_bgen_decode).  The decode writes num / g_j, g_j the column's own divisor of 2^B - 1; one fix-up
// multiply (k_dosage_scale) moves every column onto the common reduced grid, and dosage_stats computes mu, sigma exactly as for
// mih_dosage_create.  The result is the matrix genotypes.genotype_values(read_bgen(...)) builds, byte for byte.
#include "common.h"
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstring>
#include <dlfcn.h>
#include <fcntl.h>
#include <mutex>
#include <thread>
#include <unistd.h>

namespace mih {

// ---- zlib, loaded at first use (no link-time or header dependency) ----------------------------------------------------------
// BGEN stores each block's inflated length, so one call of uncompress() per block is enough.
typedef int (*uncompress_fn)(unsigned char *dest, unsigned long *dest_len, const unsigned char *src, unsigned long src_len);
enum { kZOk = 0, kZBufError = -5 };

static uncompress_fn zlib_uncompress()
{
    static const uncompress_fn fn = [] {
        void *lib = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("libz.so", RTLD_NOW | RTLD_LOCAL);
        return lib ? (uncompress_fn)dlsym(lib, "uncompress") : nullptr;
    }();
    return fn;
}

// ---- the device decode ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gcd_u32(uint32_t a, uint32_t b)
{
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}

// the two B-bit probabilities (k_AA, k_AB) of sample i, LSB first (layout 2), from a probability section of nb bytes
__device__ __forceinline__ void bgen_probs_any(const uint8_t *__restrict__ pr, int64_t nb, int B, int64_t i, uint32_t &kaa, uint32_t &kab)
{
    const int64_t bit = 2 * i * B, byte = bit >> 3;
    uint64_t w = 0;
    #pragma unroll
    for (int q = 0; q < 5; ++q)                                    // 2 B + 7 <= 39 bits
        if (byte + q < nb) w |= (uint64_t)pr[byte + q] << (8 * q);
    w >>= (bit & 7);
    const uint32_t m = (1u << B) - 1u;
    kaa = (uint32_t)w & m;
    kab = (uint32_t)(w >> B) & m;
}

// the probabilities of the 8 samples i0 .. i0 + 7 (i0 a multiple of 8, the group wholly inside the block when `whole`):
// aligned 16-byte loads for B = 8 and 16 (the probability section starts 16-byte aligned), byte extraction otherwise
template <int KIND>
__device__ __forceinline__ void bgen_group(const uint8_t *__restrict__ pr, int64_t nb, int B, int64_t i0, bool whole,
                                           uint32_t (&kaa)[8], uint32_t (&kab)[8])
{
    if (KIND == 8 && whole) {
        const uint4 q = *reinterpret_cast<const uint4 *>(pr + 2 * i0);
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        #pragma unroll
        for (int s = 0; s < 8; ++s) { const uint32_t h = w[s >> 1] >> (16 * (s & 1)); kaa[s] = h & 0xFFu; kab[s] = (h >> 8) & 0xFFu; }
    } else if (KIND == 16 && whole) {
        const uint4 *q = reinterpret_cast<const uint4 *>(pr + 4 * i0);
        const uint4 a = q[0], b = q[1];
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        #pragma unroll
        for (int s = 0; s < 8; ++s) { kaa[s] = w[s] & 0xFFFFu; kab[s] = w[s] >> 16; }
    } else {
        #pragma unroll
        for (int s = 0; s < 8; ++s) bgen_probs_any(pr, nb, B, i0 + s, kaa[s], kab[s]);
    }
}

// A staged block k (column col0 + k) is split into chunks of kBgenChunk samples, one workgroup each: a 500 000-sample column
// keeps 62 workgroups busy instead of one.  The block image sits at stg + k * slot + pre, its probability section (byte 10 + n)
// 16-byte aligned.
constexpr int64_t kBgenChunk = 8192;                               // 256 threads x 4 groups of 8 samples

// Sweep 1: check every sample of the chunk (ploidy 2; k_AA + k_AB <= 2^B - 1 where not missing: else an atomic min of the
// column index into *bad) and write the chunk's gcd of 2^B - 1 and its positive numerators num = 2 (2^B - 1) - 2 k_AA - k_AB
// (stopping at 1) to part[k * nchunk + c].
template <int KIND>
__global__ void __launch_bounds__(256)
k_bgen_scan(const uint8_t *__restrict__ stg, int64_t slot, int64_t pre, int64_t n, int B, int64_t col0, int64_t nchunk,
            uint32_t *__restrict__ part, uint32_t *__restrict__ bad)
{
    __shared__ uint32_t s_g[256];
    __shared__ int s_bad;
    const int64_t k = blockIdx.x / nchunk, c = blockIdx.x - k * nchunk;
    const uint8_t *blk = stg + k * slot + pre;
    const uint8_t *pl = blk + 8, *pr = blk + 10 + n;
    const int64_t nb = (2 * n * B + 7) / 8, hi = min(n, (c + 1) * kBgenChunk);
    const uint32_t full = (1u << B) - 1u;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    uint32_t g = full;
    bool flag = false;
    for (int64_t i0 = c * kBgenChunk + 8 * (int64_t)threadIdx.x; i0 < hi; i0 += 8 * 256) {
        const bool whole = i0 + 8 <= n;
        uint32_t kaa[8], kab[8];
        bgen_group<KIND>(pr, nb, B, i0, whole, kaa, kab);
        #pragma unroll
        for (int s = 0; s < 8; ++s) {
            if (!whole && i0 + s >= n) break;
            const uint32_t pb = pl[i0 + s];
            if ((pb & 0x3Fu) != 2u) flag = true;
            if (pb & 0x80u) continue;
            if (kaa[s] + kab[s] > full) { flag = true; continue; }
            const uint32_t num = 2u * full - 2u * kaa[s] - kab[s];
            if (num && g != 1u) g = gcd_u32(g, num);
        }
    }
    if (flag) s_bad = 1;
    s_g[threadIdx.x] = g;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_g[threadIdx.x] = gcd_u32(s_g[threadIdx.x], s_g[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[k * nchunk + c] = s_g[0];
        if (s_bad) atomicMin(bad, (uint32_t)(col0 + k));
    }
}

// Sweep 2: g_j = the gcd of the column's chunk gcds; write num / g_j as u16 (0xFFFF where the ploidy byte has bit 7 set, and in
// the pad rows up to ld), 8 rows per thread in one 16-byte store.  Chunk 0 records g_j and folds it into the gcd of every column
// decoded so far (fine[1], a compare-and-swap loop); for B = 16, once that drops below 3 (a common reduced denominator above
// 32767) the column is an atomic min into fine[0], so that the workers stop as soon as it is known.
template <int KIND>
__global__ void __launch_bounds__(256)
k_bgen_decode(const uint8_t *__restrict__ stg, int64_t slot, int64_t pre, int64_t n, int B, int64_t col0, int64_t nchunk,
              const uint32_t *__restrict__ part, uint16_t *__restrict__ Du, int64_t ld, uint32_t *__restrict__ gcol,
              uint32_t *__restrict__ fine)
{
    __shared__ uint32_t s_g[256];
    const int64_t k = blockIdx.x / nchunk, c = blockIdx.x - k * nchunk, col = col0 + k;
    const uint8_t *blk = stg + k * slot + pre;
    const uint8_t *pl = blk + 8, *pr = blk + 10 + n;
    const int64_t nb = (2 * n * B + 7) / 8, hi = min(ld, (c + 1) * kBgenChunk);
    const uint32_t full = (1u << B) - 1u;
    uint32_t g = full;
    for (int64_t q = threadIdx.x; q < nchunk; q += 256) g = gcd_u32(g, part[k * nchunk + q]);
    s_g[threadIdx.x] = g;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_g[threadIdx.x] = gcd_u32(s_g[threadIdx.x], s_g[threadIdx.x + w]);
        __syncthreads();
    }
    const uint32_t gj = s_g[0];
    if (c == 0 && threadIdx.x == 0) {
        gcol[col] = gj;
        uint32_t seen = fine[1], now = gcd_u32(seen, gj);
        while (now != seen) {
            const uint32_t was = atomicCAS(&fine[1], seen, now);
            if (was == seen) break;
            seen = was;
            now = gcd_u32(seen, gj);
        }
        if (B == 16 && now < 3u) atomicMin(&fine[0], (uint32_t)col);
    }
    uint4 *dst = reinterpret_cast<uint4 *>(Du + col * ld);
    for (int64_t i0 = c * kBgenChunk + 8 * (int64_t)threadIdx.x; i0 < hi; i0 += 8 * 256) {
        const bool whole = i0 + 8 <= n;
        uint32_t kaa[8], kab[8];
        if (i0 < n) bgen_group<KIND>(pr, nb, B, i0, whole, kaa, kab);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        #pragma unroll
        for (int s = 0; s < 8; ++s) {
            uint32_t v = 0xFFFFu;
            if (i0 + s < n && !(pl[i0 + s] & 0x80u)) {
                const int32_t num = 2 * (int32_t)full - 2 * (int32_t)kaa[s] - (int32_t)kab[s];
                v = num > 0 ? ((uint32_t)num / gj) & 0xFFFFu : 0u;
            }
            w[s >> 1] |= v << (16 * (s & 1));
        }
        dst[i0 / 8] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

template <int KIND>
static void bgen_launch(hipStream_t st, const uint8_t *dev, int64_t nblk, int64_t slot, int64_t pre, int64_t n, int B, int64_t c0,
                        int64_t nchunk, uint32_t *part, mih_mat *h, uint32_t *gcol, uint32_t *flags)
{
    const dim3 grid((unsigned)(nblk * nchunk));
    hipLaunchKernelGGL(k_bgen_scan<KIND>, grid, dim3(256), 0, st, dev, slot, pre, n, B, c0, nchunk, part, flags);
    hipLaunchKernelGGL(k_bgen_decode<KIND>, grid, dim3(256), 0, st, dev, slot, pre, n, B, c0, nchunk, part, h->Du, h->du_ld,
                       gcol, flags + 1);
}

// ---- host checks, in read_bgen's order ------------------------------------------------------------------------------------
static inline uint32_t rd32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }
static inline uint16_t rd16(const uint8_t *p) { uint16_t v; std::memcpy(&v, p, 2); return v; }

static inline int64_t prob_bytes(int64_t n, int B) { return (2 * n * B + 7) / 8; }

// The checks of the inflated block that need no pass over its samples, in read_bgen's order (the per-sample ploidy and the
// probability sums come between, on the device or in full_check).  MIH_BGEN_MALFORMED where read_bgen would fail with an
// error of its own (a block too short for what it holds): the caller falls back to it.  *B_out: the block's bit depth.
static int header_check(const uint8_t *b, int64_t len, int64_t n, int *B_out)
{
    if (len < 8) return MIH_BGEN_MALFORMED;
    if ((int64_t)rd32(b) != n || rd16(b + 4) != 2) return MIH_BGEN_HEADER;
    if (len < 8 + n) return MIH_BGEN_MALFORMED;
    if (b[6] != 2 || b[7] != 2) return MIH_BGEN_PLOIDY;
    if (len < 10 + n) return MIH_BGEN_MALFORMED;
    if (b[8 + n]) return MIH_BGEN_PHASED;
    const int B = b[9 + n];
    *B_out = B;
    if (B < 1 || B > 32) return MIH_BGEN_BITS;
    if (len < 10 + n + prob_bytes(n, B)) return MIH_BGEN_MALFORMED;
    return MIH_OK;
}

// Inflate (compression 1) or take (0) one stored block of clen bytes: the block image in out.  MIH_BGEN_CORRUPT where the
// inflated length is not the stored one, MIH_BGEN_MALFORMED where zlib refuses the stream (read_bgen fails in zlib then).
static int inflate_block(const uint8_t *src, int64_t clen, int comp, std::vector<uint8_t> &out)
{
    if (comp == 0) { out.assign(src, src + clen); return MIH_OK; }
    if (clen < 4) return MIH_BGEN_MALFORMED;
    const uint32_t dlen = rd32(src);
    out.resize(dlen);
    unsigned long got = dlen;
    const int rc = zlib_uncompress()(out.data(), &got, src + 4, (unsigned long)(clen - 4));
    if (rc == kZBufError) return MIH_BGEN_CORRUPT;               // the stream inflates to more than dlen bytes
    if (rc != kZOk) return MIH_BGEN_MALFORMED;
    if (got != dlen) return MIH_BGEN_CORRUPT;
    return MIH_OK;
}

static bool pread_full(int fd, uint8_t *dst, int64_t len, int64_t off, int64_t *got = nullptr)
{
    int64_t done = 0;
    while (done < len) {
        const ssize_t r = pread(fd, dst + done, (size_t)(len - done), (off_t)(off + done));
        if (r < 0) { if (errno == EINTR) continue; return false; }
        if (r == 0) break;
        done += r;
    }
    if (got) *got = done;
    return got ? true : done == len;
}

// Every check read_bgen makes on the block at `off`, in its order, on the host: the reason it would give (MIH_OK if none), else
// whether the block can stream after block 0's depth B0 (MIH_BGEN_DEEP, MIH_BGEN_MIXED; B0 = 0: any depth up to 16).
static int full_check(int fd, int64_t off, int comp, int64_t n, int B0, int *B_out)
{
    uint8_t lenb[4];
    int64_t got = 0;
    if (!pread_full(fd, lenb, 4, off, &got) || got < 4) return MIH_BGEN_MALFORMED;
    const int64_t clen = rd32(lenb);
    std::vector<uint8_t> raw((size_t)clen), blk;
    if (!pread_full(fd, raw.data(), clen, off + 4, &got) || got < clen) return MIH_BGEN_MALFORMED;
    int rc = inflate_block(raw.data(), clen, comp, blk);
    if (rc) return rc;
    const int64_t len = (int64_t)blk.size();
    const uint8_t *b = blk.data();
    if (len < 8) return MIH_BGEN_MALFORMED;
    if ((int64_t)rd32(b) != n || rd16(b + 4) != 2) return MIH_BGEN_HEADER;
    if (len < 8 + n) return MIH_BGEN_MALFORMED;
    if (b[6] != 2 || b[7] != 2) return MIH_BGEN_PLOIDY;
    for (int64_t i = 0; i < n; ++i) if ((b[8 + i] & 0x3F) != 2) return MIH_BGEN_PLOIDY;
    int B = 0;
    if ((rc = header_check(b, len, n, &B))) return rc;
    *B_out = B;
    const uint8_t *pr = b + 10 + n;
    const uint64_t full = (1ull << B) - 1;
    for (int64_t i = 0; i < n; ++i) {
        if (b[8 + i] & 0x80) continue;
        uint64_t kk[2];
        for (int h = 0; h < 2; ++h) {
            const int64_t bit = (2 * i + h) * B;
            uint64_t w = 0;
            for (int q = 0; q < 5 && (bit >> 3) + q < prob_bytes(n, B); ++q) w |= (uint64_t)pr[(bit >> 3) + q] << (8 * q);
            kk[h] = (w >> (bit & 7)) & full;
        }
        if (kk[0] + kk[1] > full) return MIH_BGEN_SUM;
    }
    if (B > 16) return MIH_BGEN_DEEP;
    if (B0 && B != B0) return MIH_BGEN_MIXED;
    return MIH_OK;
}

static uint32_t gcd_host(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }

struct Fd {
    int fd = -1;
    ~Fd() { if (fd >= 0) close(fd); }
};

}  // namespace mih

using namespace mih;

extern "C" {

int mih_dosage_create_bgen(const char *path, int64_t n, int64_t ncols, const int64_t *block_offset, int compression, int threads,
                           int device, mih_mat **out, int32_t *denom_out, int64_t *bad_block, int32_t *bad_what)
{
    if (!path || !block_offset || !out || !denom_out || !bad_block || !bad_what) { set_error("null argument"); return MIH_BAD_ARG; }
    *bad_block = -1; *bad_what = 0; *out = nullptr;
    if (n <= 0 || n >= (1ll << 31) || ncols <= 0 || ncols >= (1ll << 31)) { set_error("bad dimensions n=%lld ncols=%lld", (long long)n, (long long)ncols); return MIH_BAD_DIM; }
    if (compression != 0 && compression != 1) { set_error("compression must be 0 (none) or 1 (zlib), got %d", compression); return MIH_BAD_ARG; }
    if (threads < 0) { set_error("threads must be >= 0"); return MIH_BAD_ARG; }
    for (int64_t c = 0; c < ncols; ++c)
        if (block_offset[c] < 0 || (c && block_offset[c] <= block_offset[c - 1])) { set_error("block offsets must increase"); return MIH_BAD_ARG; }
    if (compression == 1 && !zlib_uncompress()) { set_error("cannot load zlib (libz.so.1) for a zlib-compressed BGEN file"); return MIH_BAD_ARG; }
    MIH_TRY(select_device(device));
    const bool trace = probe_env("MENDELIHT_INGEST_TRACE") != nullptr;           // measurement build: where the time goes
    auto tnow = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_mark = tnow();
    auto lap = [&](const char *what) { if (trace) { const double t = tnow(); fprintf(stderr, "bgen ingest: %-24s %8.2f ms\n", what, t - t_mark); t_mark = t; } };

    Fd f;
    if ((f.fd = open(path, O_RDONLY | O_CLOEXEC)) < 0) { set_error("cannot open %s: %s", path, strerror(errno)); return MIH_BAD_ARG; }
    const int fd = f.fd;
    auto refuse = [&](int64_t blk, int what) {
        *bad_block = blk; *bad_what = what;
        set_error("genotype block %lld: %s", (long long)blk,
                  what == MIH_BGEN_DEEP || what == MIH_BGEN_MIXED || what == MIH_BGEN_FINE || what == MIH_BGEN_MALFORMED
                  ? "cannot stream (see bad_what)" : "refused as read_bgen refuses it (see bad_what)");
        return MIH_BAD_ARG;
    };
    // block 0, on the host: its depth B0 sizes the staging slots
    int B0 = 0;
    if (int rc = full_check(fd, block_offset[0], compression, n, 0, &B0)) return refuse(0, rc);
    const uint32_t full = (1u << B0) - 1u;
    const int64_t need = 10 + n + prob_bytes(n, B0);
    const int64_t pre = (16 - (10 + n) % 16) % 16;                 // the probability section of every slot 16-byte aligned
    const int64_t slot = round_up(pre + need, 16);
    const int64_t chunk_bytes = 8ll << 20;                         // 8 workers pin 128 MB (two buffers each)
    int64_t per_run = std::max<int64_t>(1, chunk_bytes / slot);
    if (per_run > ncols) per_run = ncols;
    const int64_t nruns = (ncols + per_run - 1) / per_run;
    const size_t buf_bytes = (size_t)(per_run * slot);
    unsigned nth = (unsigned)threads;
    if (nth == 0) {                                                // the .bed ingest's rule: at most 8 workers
        nth = std::thread::hardware_concurrency();
        nth = nth >= 16 ? 8 : (nth >= 4 ? nth / 2 : 1);
    }
    if (const char *e = probe_env("MENDELIHT_INGEST_THREADS")) { int v = atoi(e); if (v >= 1 && v <= 64) nth = (unsigned)v; }     // measurement build
    if (nth > 64) nth = 64;
    if ((int64_t)nth > nruns) nth = (unsigned)nruns;
    const size_t staging_budget = 512ull << 20;                    // pinned (and device) staging of all workers together
    if (buf_bytes * 2 * nth > staging_budget) nth = (unsigned)std::max<size_t>(1, staging_budget / (buf_bytes * 2));

    mih_mat *h = new mih_mat();
    auto fail = [&](int code) { mih_mat_destroy(h); return code; };
    int rc = dosage_alloc(h, n, ncols, 1, device);
    if (rc) return fail(rc);
    // g_j per column; flags [0] a defect found on the device, [1] a column after which the common gcd is below 3 at B = 16, [2] the
    // gcd of the columns decoded so far; the chunk gcds of each worker's run
    DevBuf<uint32_t> gcol, flags, parts;
    const int64_t nchunk = (n + kBgenChunk - 1) / kBgenChunk;
    if ((rc = gcol.alloc((size_t)ncols)) || (rc = flags.alloc(3)) || (rc = parts.alloc((size_t)(nth * per_run * nchunk)))) return fail(rc);
    const uint32_t flags0[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, full};
    if (hipMemcpy(flags.p, flags0, sizeof(flags0), hipMemcpyHostToDevice) != hipSuccess) return fail(MIH_HIP_ERROR);
    struct Staging {
        uint8_t *pin = nullptr, *raw = nullptr; uint32_t *flag_pin = nullptr;
        ~Staging() { if (pin) (void)hipHostFree(pin); if (raw) (void)hipFree(raw); if (flag_pin) (void)hipHostFree(flag_pin); }
    } stg;
    for (;;) {                         // a failed allocation degrades to one worker before it fails the create
        const bool ok = hipHostMalloc((void **)&stg.pin, buf_bytes * 2 * nth, hipHostMallocDefault) == hipSuccess &&
                        device_malloc((void **)&stg.raw, buf_bytes * 2 * nth) == hipSuccess &&
                        hipHostMalloc((void **)&stg.flag_pin, sizeof(uint32_t) * 4 * nth, hipHostMallocDefault) == hipSuccess;
        if (ok) break;
        (void)hipGetLastError();
        if (stg.pin) { (void)hipHostFree(stg.pin); stg.pin = nullptr; }
        if (stg.raw) { (void)hipFree(stg.raw); stg.raw = nullptr; }
        if (stg.flag_pin) { (void)hipHostFree(stg.flag_pin); stg.flag_pin = nullptr; }
        if (nth == 1) { set_error("allocation of the BGEN staging buffers (2 x %zu bytes pinned + device) failed", buf_bytes); return fail(MIH_OOM); }
        nth = 1;
    }
    for (unsigned i = 0; i < 4 * nth; ++i) stg.flag_pin[i] = 0xFFFFFFFFu;
    lap("block 0 + staging");

    // the first block that cannot be taken as it is (a defect or a block that cannot stream): no run starting after it is taken
    std::atomic<int64_t> stop_at{ncols};
    std::mutex mu;
    int64_t host_blk = ncols;
    std::string err_msg;
    std::atomic<int> failed{0};
    auto stop_before = [&](int64_t b) {
        int64_t cur = stop_at.load();
        while (b < cur && !stop_at.compare_exchange_weak(cur, b)) {}
    };
    auto host_bad = [&](int64_t b) { std::lock_guard<std::mutex> g(mu); host_blk = std::min(host_blk, b); stop_before(b); };
    std::atomic<int64_t> next_run{0};
    std::atomic<unsigned> worker_no{0};
    auto worker = [&]() {
        const unsigned me = worker_no.fetch_add(1);
        struct Res {
            hipStream_t st = nullptr; hipEvent_t done[2] = {nullptr, nullptr};
            ~Res() {
                if (st) (void)hipStreamSynchronize(st);
                for (int i = 0; i < 2; ++i) if (done[i]) (void)hipEventDestroy(done[i]);
                if (st) (void)hipStreamDestroy(st);
            }
        } r;
        auto bad = [&](const char *what) { std::lock_guard<std::mutex> g(mu); if (err_msg.empty()) err_msg = what; failed.store(1); stop_before(0); };
        if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&r.st) != hipSuccess) return bad("BGEN worker: stream");
        for (int i = 0; i < 2; ++i)
            if (hipEventCreateWithFlags(&r.done[i], hipEventDisableTiming) != hipSuccess) return bad("BGEN worker: event");
        std::vector<uint8_t> raw, side;
        for (int64_t it = 0;; ++it) {
            const int64_t run = next_run.fetch_add(1);
            const int64_t c0 = run * per_run, c1 = std::min(c0 + per_run, ncols);
            if (c0 >= ncols || c0 >= stop_at.load()) break;
            const int b = (int)(it & 1);
            uint8_t *pin = stg.pin + buf_bytes * (2 * me + b), *dev = stg.raw + buf_bytes * (2 * me + b);
            uint32_t *fpin = stg.flag_pin + 4 * me + 2 * b;
            if (it >= 2) {                                         // buffers b are free again; what the device found two runs ago
                if (hipEventSynchronize(r.done[b]) != hipSuccess) return bad("BGEN worker: decode failed");
                stop_before(std::min<int64_t>(fpin[0], fpin[1]));
            }
            // the run's stored bytes in one read, from block c0's length field to the end of block c1 - 1 -- unless the offsets
            // skip variants (more than the run's staging apart): then block by block, so that no skipped block is read
            uint8_t lenb[4];
            int64_t got = 0;
            const bool piecewise = block_offset[c1 - 1] - block_offset[c0] > 2 * (int64_t)buf_bytes;
            if (!piecewise) {
                if (!pread_full(fd, lenb, 4, block_offset[c1 - 1], &got)) return bad("BGEN worker: read failed");
                const int64_t span = got < 4 ? block_offset[c1 - 1] - block_offset[c0] : block_offset[c1 - 1] + 4 + rd32(lenb) - block_offset[c0];
                raw.resize((size_t)span);
                if (!pread_full(fd, raw.data(), span, block_offset[c0], &got)) return bad("BGEN worker: read failed");
            }
            int64_t cend = c1;
            for (int64_t c = c0; c < c1; ++c) {
                int64_t o = block_offset[c] - block_offset[c0];
                int64_t lim = c + 1 < c1 ? block_offset[c + 1] - block_offset[c0] : got;
                if (piecewise) {                                   // this block alone: its length field, then its stored bytes
                    o = 0;
                    if (!pread_full(fd, lenb, 4, block_offset[c], &got)) return bad("BGEN worker: read failed");
                    raw.resize(4 + (got < 4 ? 0 : (size_t)rd32(lenb)));
                    if (!pread_full(fd, raw.data(), (int64_t)raw.size(), block_offset[c], &got)) return bad("BGEN worker: read failed");
                    lim = got;
                }
                int code = MIH_OK, B = 0;
                const uint8_t *img = nullptr;
                int64_t len = 0;
                uint8_t *dst = pin + (c - c0) * slot + pre;
                if (o + 4 > got || o + 4 + (int64_t)rd32(raw.data() + o) > std::min(lim, got)) code = MIH_BGEN_MALFORMED;
                else {
                    const int64_t clen = rd32(raw.data() + o);
                    const uint8_t *src = raw.data() + o + 4;
                    if (compression == 0) { img = src; len = clen; }
                    else if (clen < 4) code = MIH_BGEN_MALFORMED;
                    else {
                        const uint32_t dlen = rd32(src);
                        uint8_t *into = dst;
                        if ((int64_t)dlen > slot - pre) { side.resize(dlen); into = side.data(); }
                        unsigned long dl = dlen;
                        const int zr = zlib_uncompress()(into, &dl, src + 4, (unsigned long)(clen - 4));
                        code = zr == kZBufError ? MIH_BGEN_CORRUPT : (zr != kZOk ? MIH_BGEN_MALFORMED : (dl != dlen ? MIH_BGEN_CORRUPT : MIH_OK));
                        img = into; len = dlen;
                    }
                }
                if (!code) code = header_check(img, len, n, &B);
                if (!code && B > 16) code = MIH_BGEN_DEEP;
                if (!code && B != B0) code = MIH_BGEN_MIXED;
                if (code) { host_bad(c); cend = c; break; }
                if (img != dst) std::memcpy(dst, img, (size_t)need);
            }
            if (cend > c0) {
                const size_t bytes = (size_t)((cend - c0) * slot);
                if (hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, r.st) != hipSuccess) return bad("BGEN worker: H2D copy");
                uint32_t *part = parts.p + (size_t)me * (size_t)(per_run * nchunk);
                if (B0 == 8) bgen_launch<8>(r.st, dev, cend - c0, slot, pre, n, B0, c0, nchunk, part, h, gcol.p, flags.p);
                else if (B0 == 16) bgen_launch<16>(r.st, dev, cend - c0, slot, pre, n, B0, c0, nchunk, part, h, gcol.p, flags.p);
                else bgen_launch<0>(r.st, dev, cend - c0, slot, pre, n, B0, c0, nchunk, part, h, gcol.p, flags.p);
                if (hipMemcpyAsync(fpin, flags.p, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, r.st) != hipSuccess) return bad("BGEN worker: flag copy");
            }
            if (hipEventRecord(r.done[b], r.st) != hipSuccess) return bad("BGEN worker: event record");
            if (cend < c1) break;
        }
        if (hipStreamSynchronize(r.st) != hipSuccess) return bad("BGEN decode kernel failed");
    };
    if (nth <= 1) worker();
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nth; ++t) th.emplace_back(worker);
        for (auto &t : th) t.join();
    }
    if (failed.load()) { set_error("%s", err_msg.c_str()); (void)hipGetLastError(); return fail(MIH_HIP_ERROR); }
    lap("read + inflate + decode");

    // the first block in file order that is defective or cannot stream: host checks, device checks, and (B = 16) the running gcd
    uint32_t fl[2];
    if (hipMemcpy(fl, flags.p, sizeof(fl), hipMemcpyDeviceToHost) != hipSuccess) return fail(MIH_HIP_ERROR);
    int64_t first = std::min<int64_t>({host_blk, (int64_t)fl[0], (int64_t)fl[1]});
    std::vector<uint32_t> g((size_t)ncols);
    const int64_t decoded = std::min<int64_t>(first, ncols);
    if (decoded > 0 && hipMemcpy(g.data(), gcol.p, sizeof(uint32_t) * (size_t)decoded, hipMemcpyDeviceToHost) != hipSuccess) return fail(MIH_HIP_ERROR);
    uint32_t G = full;
    for (int64_t c = 0; c < decoded; ++c) {
        G = gcd_host(G, g[(size_t)c]);
        if (full / G > 32767u) { first = c; break; }              // only at B = 16: the common grid finer than 1/32767
    }
    if (first < ncols) {
        int B = 0;
        const int why = full_check(fd, block_offset[first], compression, n, B0, &B);
        mih_mat_destroy(h);
        return refuse(first, why ? why : MIH_BGEN_FINE);
    }
    dosage_rescale(h, gcol.p, G, 1u);
    h->denom = (int32_t)(full / G);
    if ((rc = dosage_stats(h))) return fail(rc);
    lap("fix-up + statistics");
    *denom_out = h->denom;
    *out = h;
    return MIH_OK;
}

}  // extern "C"
