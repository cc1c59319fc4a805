// vcf.hip -- VCF text (plain, gzip, BGZF) streamed from disk into the 16-bit dosage matrix; the GPU tokenises the sample fields.
//
// Pass 1 (mih_vcf_open, host only): the container is found from the file's first bytes, the inflated text is scanned once for
// the #CHROM line (n), the number of records, the longest line, and a table of chunks: runs of whole lines of at most
// max(chunk_bytes, longest line) bytes, each with the inflated offset it starts at and the index of its first record.  BGZF
// blocks are inflated in parallel, batch by batch, and indexed (file offset, inflated offset); a plain gzip file is one serial
// stream.  Pass 2 (mih_dosage_create_vcf): workers with their own stream, two pinned and two device buffers (the scheme of
// bgen.hip) take chunks from one queue -- pread (text), inflate the blocks that cover the chunk (BGZF), or, one worker alone,
// inflate the stream on (gzip) -- split the first nine fields of every record on the host (CHROM..ALT kept for mih_vcf_meta,
// k from FORMAT) and hand the device {first sample byte, line end, k, column} per record.  k_vcf_count counts the tabs of every
// 4 KB segment of a record's sample fields; k_vcf_parse gives every tab its sample index, skips k colons behind it, parses the
// GT or DS token and writes one u16.  DS numerators are over 10^4; the running gcd of 10^4 and every positive numerator
// gives the matrix's own reduced grid.  Whatever is outside the grammar is an atomic min of (record, reason): the caller hands the
// file to the host reader.  mih_snp_create_vcf is the same pass 2 for hard calls: k_vcf_parse fills a small u16 panel of the chunk's
// records instead of the matrix, and the pack kernel of snp.hip, queued behind it, writes those columns of a 2-bit image.
#include "common.h"
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <dlfcn.h>
#include <fcntl.h>
#include <mutex>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>

namespace mih {

// ---- zlib's stream interface, loaded at first use (no link-time or header dependency) ------------------------------------
struct ZStream {                                                   // z_stream of zlib 1.x
    const unsigned char *next_in; unsigned avail_in; unsigned long total_in;
    unsigned char *next_out; unsigned avail_out; unsigned long total_out;
    const char *msg; void *state; void *zalloc; void *zfree; void *opaque;
    int data_type; unsigned long adler; unsigned long reserved;
};
enum { kZStreamEnd = 1, kZNoFlush = 0, kZFinish = 4, kZGzip = 15 + 16 };
struct ZLib {
    int (*init2)(ZStream *, int, const char *, int) = nullptr;
    int (*inflate)(ZStream *, int) = nullptr;
    int (*reset)(ZStream *) = nullptr;
    int (*end)(ZStream *) = nullptr;
    bool ok() const { return init2 && inflate && reset && end; }
};
static const ZLib &zlib_stream()
{
    static const ZLib z = [] {
        ZLib l;
        void *lib = dlopen("libz.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("libz.so", RTLD_NOW | RTLD_LOCAL);
        if (lib) {
            l.init2 = (int (*)(ZStream *, int, const char *, int))dlsym(lib, "inflateInit2_");
            l.inflate = (int (*)(ZStream *, int))dlsym(lib, "inflate");
            l.reset = (int (*)(ZStream *))dlsym(lib, "inflateReset");
            l.end = (int (*)(ZStream *))dlsym(lib, "inflateEnd");
        }
        return l;
    }();
    return z;
}
struct Inflater {                                                  // one gzip-wrapped inflate state (header, CRC and length checked)
    ZStream s;
    bool live = false;
    Inflater() { std::memset(&s, 0, sizeof(s)); }
    ~Inflater() { if (live) zlib_stream().end(&s); }
    bool init() { live = zlib_stream().init2(&s, kZGzip, "1.2.11", (int)sizeof(ZStream)) == 0; return live; }
    // one whole member src[0, len) into dst[0, cap): its inflated length, or -1
    int64_t member(const uint8_t *src, size_t len, uint8_t *dst, size_t cap)
    {
        uint8_t none;
        if (cap == 0) { dst = &none; cap = 1; }                      // an empty member (the BGZF EOF block) still needs somewhere to write
        if (zlib_stream().reset(&s) != 0) return -1;
        s.next_in = src; s.avail_in = (unsigned)len; s.next_out = dst; s.avail_out = (unsigned)cap;
        if (zlib_stream().inflate(&s, kZFinish) != kZStreamEnd || s.avail_in != 0) return -1;
        return (int64_t)(cap - s.avail_out);
    }
};

static bool pread_all(int fd, uint8_t *dst, int64_t len, int64_t off, int64_t *got)
{
    int64_t done = 0;
    while (done < len) {
        const ssize_t r = pread(fd, dst + done, (size_t)(len - done), (off_t)(off + done));
        if (r < 0) { if (errno == EINTR) continue; return false; }
        if (r == 0) break;
        done += r;
    }
    *got = done;
    return true;
}

static inline uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
static inline uint32_t le32(const uint8_t *p) { uint32_t v; std::memcpy(&v, p, 4); return v; }

// The size of the BGZF block whose gzip header starts at h (avail bytes readable): BSIZE + 1 from the BC subfield of the extra
// field, 0 where the header is no gzip header with one.
static int64_t bgzf_block_size(const uint8_t *h, int64_t avail)
{
    if (avail < 12 || h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return 0;
    const int64_t xlen = le16(h + 10);
    if (12 + xlen > avail) return 0;
    for (int64_t q = 12; q + 4 <= 12 + xlen;) {
        const int64_t slen = le16(h + q + 2);
        if (h[q] == 66 && h[q + 1] == 67 && slen == 2 && q + 6 <= 12 + xlen) return (int64_t)le16(h + q + 4) + 1;
        q += 4 + slen;
    }
    return 0;
}

struct VcfChunk { int64_t off, rec0; };                            // a run of whole lines: inflated offset, index of its first record
struct VcfBlock { int64_t foff, ioff; uint32_t csize, isize; };    // a BGZF block: file offset, inflated offset, stored and inflated size

}  // namespace mih

using namespace mih;

struct mih_vcf {
    std::string path;
    int fd = -1;
    int32_t container = 0;                                         // 0 text, 1 gzip, 2 BGZF
    int64_t n = 0, nrecords = 0, longest = 0, total = 0, chunk_bytes = 0, max_chunk = 0, max_chunk_records = 0;
    std::string header, meta;
    std::vector<VcfChunk> chunks;                                  // and a sentinel {total, nrecords}
    std::vector<VcfBlock> blocks;
    ~mih_vcf() { if (fd >= 0) close(fd); }
};

namespace mih {

// a '\r' or a byte >= 0x80 among len bytes (the # lines: the host reader splits at the one and decodes the other its own way)
static bool cr_or_high(const uint8_t *b, int64_t len)
{
    uint8_t any = 0;
    for (int64_t i = 0; i < len; ++i) any |= (uint8_t)((b[i] & 0x80) | (b[i] == '\r'));
    return any != 0;
}

// ---- pass 1: the line scan of the inflated text --------------------------------------------------------------------------
struct LineScan {
    mih_vcf *v;
    int64_t off = 0, line_start = 0, linelen = 0, chunk_start = 0, chunk_rec0 = 0, nrec = 0;
    int kind = 0;                                                  // 0 record, 1 ## line, 2 the #CHROM line, 3 '#' seen, next byte pending
    bool have_header = false;
    int what = 0;                                                  // MIH_VCF_* of the first trouble, at record nrec
    explicit LineScan(mih_vcf *v_) : v(v_) {}

    void end_line(int64_t next)                                    // the line [line_start, next) ends (next: where the following one starts)
    {
        if (linelen == 0) {                                        // an empty line is a (ragged) record
            line_start = next - 1; kind = 0;
            if (!have_header) { what = MIH_VCF_HEADER; return; }
        }
        if (kind == 3) { kind = 2; if (have_header) { what = MIH_VCF_HEADER; return; } v->header = "#"; }
        if (kind == 2) have_header = true;
        if (kind == 0) ++nrec;
        v->longest = std::max(v->longest, linelen);
        if (next - chunk_start > v->chunk_bytes && line_start > chunk_start) {      // the chunk ends before this line
            v->chunks.push_back({chunk_start, chunk_rec0});
            chunk_start = line_start; chunk_rec0 = nrec - (kind == 0 ? 1 : 0);
        }
        if (next - chunk_start >= v->chunk_bytes) {
            v->chunks.push_back({chunk_start, chunk_rec0});
            chunk_start = next; chunk_rec0 = nrec;
        }
        linelen = 0; kind = 0;
    }
    void feed(const uint8_t *buf, int64_t len)
    {
        int64_t p = 0;
        while (p < len && !what) {
            if (linelen < 2 && buf[p] != '\n') {                   // the first two bytes of a line decide its kind
                const uint8_t c = buf[p];
                if (linelen == 0) {
                    line_start = off + p; kind = c == '#' ? 3 : 0;
                    if (kind == 0 && !have_header) { what = MIH_VCF_HEADER; return; }
                } else if (kind == 3) {
                    kind = c == '#' ? 1 : 2;
                    if (kind == 2) {
                        if (have_header) { what = MIH_VCF_HEADER; return; }
                        v->header.assign("#"); v->header.push_back((char)c);
                    }
                } else if (kind == 2) v->header.push_back((char)c);
                if (kind != 0 && (c == '\r' || c >= 0x80)) { what = MIH_VCF_HEADER; return; }
                ++linelen; ++p;
                continue;
            }
            const uint8_t *nl = (const uint8_t *)memchr(buf + p, '\n', (size_t)(len - p));
            const int64_t seg = (nl ? nl - buf : len) - p;
            if (kind != 0 && cr_or_high(buf + p, seg)) { what = MIH_VCF_HEADER; return; }
            if (kind == 2) v->header.append((const char *)buf + p, (size_t)seg);
            linelen += seg; p += seg;
            if (nl) { ++p; end_line(off + p); }
        }
        off += len;
    }
    void finish()
    {
        if (!what && linelen > 0) end_line(off);
        if (!what && !have_header) what = MIH_VCF_HEADER;
        if (what) return;
        if (chunk_start < off) v->chunks.push_back({chunk_start, chunk_rec0});
        v->chunks.push_back({off, nrec});
        v->total = off; v->nrecords = nrec;
        for (size_t c = 0; c + 1 < v->chunks.size(); ++c) {
            v->max_chunk = std::max(v->max_chunk, v->chunks[c + 1].off - v->chunks[c].off);
            v->max_chunk_records = std::max(v->max_chunk_records, v->chunks[c + 1].rec0 - v->chunks[c].rec0);
        }
    }
};

// ---- pass 2, host side: the text of one chunk -------------------------------------------------------------------------------
// One per worker.  fill(c, txt): the inflated bytes of chunk c into txt -- pread (text), the BGZF blocks that cover the chunk
// (a block wholly inside inflates straight into txt, one cut by a chunk border through a side buffer), or the gzip stream carried
// on from where the chunk before ended (so a gzip file's chunks come in order, from chunk 0, to ONE reader).  false: the file
// is no longer what pass 1 read.
struct ChunkReader {
    const mih_vcf *v;
    Inflater z;
    std::vector<uint8_t> raw, side;
    int64_t gz_off = 0;                                            // gzip: the file offset read up to, the member state
    bool gz_ended = false;
    explicit ChunkReader(const mih_vcf *v_) : v(v_) {}
    bool init()
    {
        if (v->container && !z.init()) return false;
        if (v->container == 1) { raw.resize((size_t)(1 << 20)); z.s.avail_in = 0; }
        if (v->container == 2) side.resize((size_t)65536);
        return true;
    }
    bool fill(int64_t c, uint8_t *txt)
    {
        const int64_t s0 = v->chunks[(size_t)c].off, len = v->chunks[(size_t)c + 1].off - s0;
        int64_t got = 0;
        if (v->container == 0) return pread_all(v->fd, txt, len, s0, &got) && got == len;
        if (v->container == 1) {
            z.s.next_out = txt; z.s.avail_out = (unsigned)len;
            while (z.s.avail_out) {
                if (z.s.avail_in == 0) {
                    if (!pread_all(v->fd, raw.data(), (int64_t)raw.size(), gz_off, &got) || got == 0) return false;
                    gz_off += got;
                    z.s.next_in = raw.data(); z.s.avail_in = (unsigned)got;
                }
                if (gz_ended) { if (zlib_stream().reset(&z.s) != 0) return false; gz_ended = false; }
                const int zr = zlib_stream().inflate(&z.s, kZNoFlush);
                if (zr != 0 && zr != kZStreamEnd) return false;
                if (zr == kZStreamEnd) gz_ended = true;
            }
            return true;
        }
        const auto &B = v->blocks;
        const size_t b0 = (size_t)(std::upper_bound(B.begin(), B.end(), s0, [](int64_t o, const VcfBlock &x) { return o < x.ioff; }) - B.begin()) - 1;
        size_t b1 = b0;
        while (b1 + 1 < B.size() && B[b1 + 1].ioff < s0 + len) ++b1;
        const int64_t span = B[b1].foff + B[b1].csize - B[b0].foff;
        raw.resize((size_t)span);
        if (!pread_all(v->fd, raw.data(), span, B[b0].foff, &got) || got != span) return false;
        for (size_t q = b0; q <= b1; ++q) {
            const uint8_t *src = raw.data() + (B[q].foff - B[b0].foff);
            if (B[q].ioff >= s0 && B[q].ioff + B[q].isize <= s0 + len) {
                if (z.member(src, B[q].csize, txt + (B[q].ioff - s0), B[q].isize) != (int64_t)B[q].isize) return false;
            } else {
                if (z.member(src, B[q].csize, side.data(), side.size()) != (int64_t)B[q].isize) return false;
                const int64_t lo = std::max(s0, B[q].ioff), hi = std::min(s0 + len, B[q].ioff + (int64_t)B[q].isize);
                if (hi > lo) std::memcpy(txt + (lo - s0), side.data() + (lo - B[q].ioff), (size_t)(hi - lo));
            }
        }
        return true;
    }
};

static unsigned default_workers(int threads)                        // the .bed ingest's rule: at most 8 workers
{
    unsigned nth = (unsigned)threads;
    if (nth == 0) {
        nth = std::thread::hardware_concurrency();
        nth = nth >= 16 ? 8 : (nth >= 4 ? nth / 2 : 1);
    }
    return std::min(nth, 64u);
}

// ---- the device tokeniser -------------------------------------------------------------------------------------------------
struct VcfRec { uint32_t first, end; int32_t k, col; uint32_t seg0; };   // sample fields [first, end) of the chunk buffer; first segment
constexpr uint32_t kVcfSeg = 4096;                                 // 256 threads x 16 bytes

__device__ __forceinline__ uint32_t zero_bytes(uint32_t x)         // 0x80 in every byte of x that is 0
{
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
__device__ __forceinline__ uint32_t byte_bits(uint32_t t)          // 0x80 flags of 4 bytes -> 4 bits
{
    return ((t >> 7) & 1u) | ((t >> 14) & 2u) | ((t >> 21) & 4u) | ((t >> 28) & 8u);
}
// of the 16 bytes q at buffer position pos: the bits of those inside [first, end) that are a tab; ugly: a '\r' or a byte >= 0x80
__device__ __forceinline__ uint32_t tab_mask(const uint4 &q, uint32_t pos, uint32_t first, uint32_t end, bool &ugly)
{
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    uint32_t tabs = 0, bad = 0;
    #pragma unroll
    for (int j = 0; j < 4; ++j) {
        tabs |= byte_bits(zero_bytes(w[j] ^ 0x09090909u)) << (4 * j);
        bad |= byte_bits(zero_bytes(w[j] ^ 0x0D0D0D0Du) | (w[j] & 0x80808080u)) << (4 * j);
    }
    const uint32_t lo = first > pos ? min(first - pos, 16u) : 0u, hi = min(end - pos, 16u);
    const uint32_t valid = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
    ugly = (bad & valid) != 0;
    return tabs & valid;
}
// the record of workgroup b: the last r with rec[r].seg0 <= b (rec[nrec] is a sentinel)
__device__ __forceinline__ int record_of(const VcfRec *__restrict__ rec, int nrec, uint32_t b)
{
    int lo = 0, hi = nrec - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (rec[mid].seg0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ void flag_bad(unsigned long long *bad, int64_t record, int what)
{
    atomicMin(bad, ((unsigned long long)record << 8) | (unsigned long long)what);
}

// Sweep 1: the tabs of segment s of record r (bytes [a0 + s kVcfSeg, ...) of the chunk, a0 = first rounded down to 16) into
// segcnt[seg0 + s]; a '\r' or a non-ASCII byte among the sample fields flags the record.
__global__ void __launch_bounds__(256)
k_vcf_count(const uint8_t *__restrict__ txt, const VcfRec *__restrict__ rec, int nrec, int64_t rec_base,
            uint32_t *__restrict__ segcnt, unsigned long long *__restrict__ bad)
{
    __shared__ uint32_t s_cnt, s_ugly;
    const int r = record_of(rec, nrec, blockIdx.x);
    const VcfRec R = rec[r];
    if (threadIdx.x == 0) { s_cnt = 0; s_ugly = 0; }
    __syncthreads();
    const uint32_t pos = (R.first & ~15u) + (blockIdx.x - R.seg0) * kVcfSeg + threadIdx.x * 16u;
    if (pos < R.end) {
        bool ugly;
        const uint32_t m = tab_mask(*reinterpret_cast<const uint4 *>(txt + pos), pos, R.first, R.end, ugly);
        if (m) atomicAdd(&s_cnt, (uint32_t)__popc(m));
        if (ugly) s_ugly = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        segcnt[blockIdx.x] = s_cnt;
        if (s_ugly) flag_bad(bad, rec_base + R.col, MIH_VCF_TOKEN);
    }
}

// the value of a token: 0 .. 20000, 0xFFFF missing, or a reason (MIH_VCF_*) in the upper half
template <typename At>
__device__ __forceinline__ uint32_t parse_gt(At at, uint32_t q, uint32_t end)
{
    uint32_t c[4];
    int len = 0;
    for (; len < 4 && q + len < end; ++len) {
        c[len] = at(q + len);
        if (c[len] == ':' || c[len] == '\t') break;
    }
    if (len == 0) return 0xFFFFu;
    if (len != 1 && len != 3) return (uint32_t)MIH_VCF_TOKEN << 16;
    uint32_t v = 0;
    bool miss = false;
    for (int a = 0; a < len; a += 2) {
        if (c[a] == '.') miss = true;
        else if (c[a] == '1') ++v;
        else if (c[a] != '0') return (uint32_t)MIH_VCF_TOKEN << 16;
    }
    if (len == 3 && c[1] != '/' && c[1] != '|') return (uint32_t)MIH_VCF_TOKEN << 16;
    return miss ? 0xFFFFu : v;
}

template <typename At>
__device__ __forceinline__ uint32_t parse_ds(At at, uint32_t q, uint32_t end)
{
    uint32_t ip = 0, fr = 0;
    int nint = 0, nfrac = 0, len = 0;
    bool dot = false, deep = false;
    for (; q + len < end; ++len) {
        const uint32_t ch = at(q + len);
        if (ch == ':' || ch == '\t') break;
        if (len >= 32) return (uint32_t)MIH_VCF_TOKEN << 16;
        if (ch == '.') { if (dot) return (uint32_t)MIH_VCF_TOKEN << 16; dot = true; continue; }
        const uint32_t d = ch - '0';
        if (d > 9u) return (uint32_t)MIH_VCF_TOKEN << 16;
        if (!dot) { ip = min(ip * 10u + d, 1000u); ++nint; }
        else {
            if (nfrac < 4) fr = fr * 10u + d; else if (d) deep = true;
            ++nfrac;
        }
    }
    if (len == 0 || (len == 1 && dot)) return 0xFFFFu;
    if (nint == 0 && nfrac == 0) return (uint32_t)MIH_VCF_TOKEN << 16;
    if (deep) return (uint32_t)MIH_VCF_DECIMALS << 16;
    for (; nfrac < 4; ++nfrac) fr *= 10u;
    const uint32_t v = ip * 10000u + fr;
    if (v > 20000u) return (uint32_t)MIH_VCF_RANGE << 16;
    return v;
}

__device__ __forceinline__ uint32_t gcd_u32v(uint32_t a, uint32_t b)
{
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}

// Sweep 2: the segment staged in LDS; every tab gets its sample index (the record's tabs in the segments before, a workgroup
// scan, its rank among the thread's own); the thread behind a tab skips k colons, parses the token (reading on past its 16
// bytes and past the segment, never past the line end) and writes Du[col ld + i].  Sample 0 belongs to thread 0 of segment 0,
// the pad rows to whoever holds sample n - 1.  The record's last segment checks that it has n - 1 tabs.  FIELD 1 (DS): the
// workgroup's gcd of 10^4 and its positive numerators is folded into *gcdp (compare-and-swap).
template <int FIELD>
__global__ void __launch_bounds__(256)
k_vcf_parse(const uint8_t *__restrict__ txt, const VcfRec *__restrict__ rec, int nrec, int64_t rec_base,
            const uint32_t *__restrict__ segcnt, int64_t n, uint16_t *__restrict__ Du, int64_t ld,
            unsigned long long *__restrict__ bad, uint32_t *__restrict__ gcdp)
{
    __shared__ uint4 s_txt[256];
    __shared__ uint32_t s_wave[4], s_base, s_m2, s_m5, s_what;
    const int r = record_of(rec, nrec, blockIdx.x);
    const VcfRec R = rec[r];
    const uint32_t s = blockIdx.x - R.seg0, nseg = rec[r + 1].seg0 - R.seg0;
    const uint32_t seg_lo = (R.first & ~15u) + s * kVcfSeg, pos = seg_lo + threadIdx.x * 16u;
    if (threadIdx.x == 0) { s_base = 0; s_m2 = 4; s_m5 = 4; s_what = 0xFFFFFFFFu; }
    __syncthreads();
    uint32_t part = 0;
    for (uint32_t q = threadIdx.x; q < s; q += 256) part += segcnt[R.seg0 + q];
    if (part) atomicAdd(&s_base, part);
    uint32_t m = 0;
    uint4 mine = make_uint4(0u, 0u, 0u, 0u);
    if (pos < R.end) {
        bool ugly;
        mine = *reinterpret_cast<const uint4 *>(txt + pos);
        m = tab_mask(mine, pos, R.first, R.end, ugly);
    }
    s_txt[threadIdx.x] = mine;
    // exclusive scan of the threads' tab counts: within the wave by shuffles, across the 4 waves through LDS
    const uint32_t cnt = (uint32_t)__popc(m), lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = cnt;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if ((int)lane >= d) inc += up;
    }
    if (lane == 63u) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = s_base + inc - cnt, total = s_base;
    #pragma unroll
    for (uint32_t w = 0; w < 4; ++w) { if (w < wave) before += s_wave[w]; total += s_wave[w]; }
    if (threadIdx.x == 0 && s + 1 == nseg && (int64_t)total != n - 1) flag_bad(bad, rec_base + R.col, MIH_VCF_RAGGED);

    const uint8_t *lds = reinterpret_cast<const uint8_t *>(s_txt);
    auto at = [&](uint32_t q) -> uint32_t { return q - seg_lo < kVcfSeg ? lds[q - seg_lo] : txt[q]; };
    uint16_t *dst = Du + (int64_t)R.col * ld;
    uint32_t m2 = 4, m5 = 4, what = 0;
    auto token = [&](int64_t i, uint32_t q) {
        if (i >= n) return;                                        // more than n fields: the record is flagged above
        bool missing = false;
        for (int c = R.k; c > 0;) {                                // the k-th colon of the field, if it has one
            if (q >= R.end) { missing = true; break; }
            const uint32_t ch = at(q);
            if (ch == '\t') { missing = true; break; }
            ++q;
            if (ch == ':') --c;
        }
        uint32_t v = missing ? 0xFFFFu : (FIELD ? parse_ds(at, q, R.end) : parse_gt(at, q, R.end));
        if (v >> 16) { what = what ? min(what, v >> 16) : (v >> 16); v = 0xFFFFu; }
        if (FIELD && v && v != 0xFFFFu) {
            m2 = min(m2, (uint32_t)__ffs(v) - 1u);
            uint32_t f = 0;
            if (m5) { f = v % 5u ? 0u : (v % 25u ? 1u : (v % 125u ? 2u : (v % 625u ? 3u : 4u))); m5 = min(m5, f); }
        }
        dst[i] = (uint16_t)v;
        if (i == n - 1) for (int64_t pad = n; pad < ld; ++pad) dst[pad] = 0xFFFFu;
    };
    if (s == 0 && threadIdx.x == 0) token(0, R.first);
    for (uint32_t rest = m, rank = 0; rest; rest &= rest - 1u, ++rank)
        token((int64_t)before + rank + 1, pos + (uint32_t)__ffs(rest));
    if (FIELD && (m2 < 4u || m5 < 4u)) { atomicMin(&s_m2, m2); atomicMin(&s_m5, m5); }
    if (what) atomicMin(&s_what, what);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_what != 0xFFFFFFFFu) flag_bad(bad, rec_base + R.col, (int)s_what);
        if (FIELD && (s_m2 < 4u || s_m5 < 4u)) {
            uint32_t g = 1u << s_m2;
            for (uint32_t e = 0; e < s_m5; ++e) g *= 5u;
            uint32_t seen = *(volatile uint32_t *)gcdp, now = gcd_u32v(seen, g);
            while (now != seen) {
                const uint32_t was = atomicCAS(gcdp, seen, now);
                if (was == seen) break;
                seen = was;
                now = gcd_u32v(seen, g);
            }
        }
    }
}

// every numerator of the matrix divided by g, the gcd of 10^4 and all of them (0xFFFF stays): one block per column
__global__ void __launch_bounds__(256)
k_vcf_reduce(uint16_t *__restrict__ X, int64_t ld, uint32_t g)
{
    uint4 *cx = reinterpret_cast<uint4 *>(X + (int64_t)blockIdx.x * ld);
    for (int64_t i = threadIdx.x; i < ld / 8; i += 256) {
        const uint4 q = cx[i];
        uint32_t w[4] = {q.x, q.y, q.z, q.w};
        #pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t lo = w[k] & 0xFFFFu, hi = w[k] >> 16;
            w[k] = (lo == 0xFFFFu ? lo : lo / g) | ((hi == 0xFFFFu ? hi : hi / g) << 16);
        }
        cx[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

static const char *vcf_reason(int what)
{
    switch (what) {
    case MIH_VCF_RAGGED: return "not 9 + n tab-separated fields";
    case MIH_VCF_TOKEN: return "a token outside the streamed grammar";
    case MIH_VCF_RANGE: return "a dosage above 2";
    case MIH_VCF_DECIMALS: return "more than 4 decimals";
    case MIH_VCF_NOKEY: return "the wanted key is not in FORMAT";
    case MIH_VCF_MULTIALLELIC: return "a comma in ALT";
    case MIH_VCF_HEADER: return "header lines other than ASCII ## lines and one ASCII #CHROM line before the records";
    case MIH_VCF_IO: return "not a regular file that can be opened and read";
    case MIH_VCF_NOT_HARD_CALL: return "a DS value other than 0, 1 or 2: not a hard call";
    case MIH_VCF_CONTAINER: return "a container that is not what the file name says, does not inflate or is truncated";
    }
    return "?";
}

}  // namespace mih

extern "C" {

int mih_vcf_open(const char *path, int threads, int64_t chunk_bytes, mih_vcf **out, int64_t *bad_record, int32_t *bad_what)
{
    if (!path || !out || !bad_record || !bad_what) { set_error("null argument"); return MIH_BAD_ARG; }
    *out = nullptr; *bad_record = -1; *bad_what = 0;
    if (threads < 0 || chunk_bytes < 0 || chunk_bytes > (1ll << 30)) { set_error("threads must be >= 0 and chunk_bytes in [0, 2^30]"); return MIH_BAD_ARG; }
    std::unique_ptr<mih_vcf> v(new mih_vcf());
    v->path = path;
    v->chunk_bytes = chunk_bytes ? chunk_bytes : (8ll << 20);      // the BGEN run size
    LineScan scan(v.get());
    auto refuse = [&](int64_t record, int what) {
        *bad_record = record; *bad_what = what;
        set_error("%s: record %lld: %s", path, (long long)(record + 1), vcf_reason(what));
        return MIH_BAD_ARG;
    };
    // Only a regular file is opened: a missing path, a directory, a pipe (which the host reader can iterate, and which must not
    // lose its bytes to this scan) or an unreadable file is the host reader's to take or to refuse in its own words.
    struct stat sb;
    if (stat(path, &sb) != 0 || !S_ISREG(sb.st_mode)) return refuse(0, MIH_VCF_IO);
    if ((v->fd = open(path, O_RDONLY | O_CLOEXEC)) < 0 || fstat(v->fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return refuse(0, MIH_VCF_IO);
    const int64_t fsize = sb.st_size;
    // the container, from the bytes; the host reader opens by name, so the two have to agree
    uint8_t head[64];
    int64_t got = 0;
    if (!pread_all(v->fd, head, sizeof(head), 0, &got)) return refuse(scan.nrec, MIH_VCF_IO);
    const bool gz_name = v->path.size() >= 3 && v->path.compare(v->path.size() - 3, 3, ".gz") == 0;
    const bool gz = got >= 2 && head[0] == 0x1f && head[1] == 0x8b;
    if (gz != gz_name) return refuse(0, MIH_VCF_CONTAINER);
    v->container = !gz ? 0 : (bgzf_block_size(head, got) ? 2 : 1);
    if (gz && !zlib_stream().ok()) return refuse(0, MIH_VCF_CONTAINER);

    const int64_t kIn = 4ll << 20;
    if (v->container == 0) {
        std::vector<uint8_t> buf((size_t)kIn);
        for (int64_t off = 0; off < fsize && !scan.what;) {
            if (!pread_all(v->fd, buf.data(), kIn, off, &got) || got == 0) return refuse(scan.nrec, MIH_VCF_IO);
            scan.feed(buf.data(), got);
            off += got;
        }
    } else if (v->container == 1) {                                // one serial stream, member after member
        std::vector<uint8_t> in((size_t)(1 << 20)), outb((size_t)kIn);
        Inflater z;
        if (!z.init()) return refuse(0, MIH_VCF_CONTAINER);
        int64_t off = 0;
        bool ended = false;                                        // at a member's end
        z.s.avail_in = 0;
        while (!scan.what) {
            if (z.s.avail_in == 0) {
                if (!pread_all(v->fd, in.data(), (int64_t)in.size(), off, &got)) return refuse(scan.nrec, MIH_VCF_IO);
                if (got == 0) { if (!ended) return refuse(scan.nrec, MIH_VCF_CONTAINER); break; }   // truncated inside a member
                off += got;
                z.s.next_in = in.data(); z.s.avail_in = (unsigned)got;
            }
            if (ended) { if (zlib_stream().reset(&z.s) != 0) return refuse(scan.nrec, MIH_VCF_CONTAINER); ended = false; }
            z.s.next_out = outb.data(); z.s.avail_out = (unsigned)outb.size();
            const int rc = zlib_stream().inflate(&z.s, kZNoFlush);
            if (rc != 0 && rc != kZStreamEnd) return refuse(scan.nrec, MIH_VCF_CONTAINER);
            scan.feed(outb.data(), (int64_t)outb.size() - z.s.avail_out);
            if (rc == kZStreamEnd) ended = true;
        }
    } else {                                                       // BGZF: batches of blocks, inflated in parallel, scanned in order
        // Two batch buffers: while the workers inflate one batch, this thread scans the one before.
        const int64_t kBatch = 256;
        const unsigned nth = std::min(default_workers(threads), 8u);       // started anew for each batch: some 10 us per thread beside 16 MB to inflate
        std::vector<uint8_t> in[2], outb[2];
        std::vector<Inflater> zs(nth);
        for (auto &z : zs) if (!z.init()) return refuse(0, MIH_VCF_CONTAINER);
        int64_t foff = 0, ioff = 0, prev_len = -1;
        int64_t guess = 4ll << 20;                                 // stored bytes to read for a batch: a little more than the last one took
        for (int cur = 0;; cur ^= 1) {
            const bool more = foff < fsize && !scan.what;
            size_t b0 = 0, nb = 0;
            int64_t q = 0, iq = 0;
            if (more) {
                // the batch's blocks, walked by their sizes, out of one read: up to 256 blocks, fewer where the read ends first (a block is at most 64 KB)
                const int64_t want = std::min(fsize - foff, guess);
                in[cur].resize((size_t)want);
                outb[cur].resize((size_t)(kBatch << 16));
                if (!pread_all(v->fd, in[cur].data(), want, foff, &got) || got != want) return refuse(scan.nrec, MIH_VCF_IO);
                b0 = v->blocks.size();
                while (q < want && (int64_t)(v->blocks.size() - b0) < kBatch) {
                    const int64_t bs = bgzf_block_size(in[cur].data() + q, want - q);
                    if ((bs == 0 || q + bs > want) && foff + want < fsize && v->blocks.size() > b0) break;   // cut by the batch's end: next batch
                    if (bs < 26 || q + bs > want) return refuse(scan.nrec, MIH_VCF_CONTAINER);
                    const uint32_t isize = le32(in[cur].data() + q + bs - 4);
                    if (isize > 65536u) return refuse(scan.nrec, MIH_VCF_CONTAINER);
                    v->blocks.push_back({foff + q, ioff + iq, (uint32_t)bs, isize});
                    q += bs; iq += isize;
                }
                nb = v->blocks.size() - b0;
                if (nb == 0) return refuse(scan.nrec, MIH_VCF_CONTAINER);
            }
            std::atomic<size_t> next{0};
            std::atomic<int> failed{0};
            auto work = [&](unsigned me) {
                for (size_t b; (b = next.fetch_add(1)) < nb;) {
                    const VcfBlock &B = v->blocks[b0 + b];
                    if (zs[me].member(in[cur].data() + (B.foff - foff), B.csize, outb[cur].data() + (B.ioff - ioff), B.isize) != (int64_t)B.isize) failed.store(1);
                }
            };
            std::vector<std::thread> th;
            const unsigned use = (unsigned)std::min<size_t>(nth, (nb + 15) / 16);
            for (unsigned t = 0; t < use; ++t) th.emplace_back(work, t);
            if (prev_len >= 0) scan.feed(outb[cur ^ 1].data(), prev_len);
            for (auto &t : th) t.join();
            if (failed.load()) return refuse(scan.nrec, MIH_VCF_CONTAINER);
            if (!more) break;
            prev_len = iq;
            foff += q; ioff += iq;
            guess = std::min<int64_t>(kBatch << 16, q + q / 4 + (1 << 17));
        }
    }
    scan.finish();
    if (scan.what) return refuse(scan.nrec, scan.what);
    // n from the #CHROM line, as the host reader splits it
    int64_t tabs = 0;
    for (char c : v->header) tabs += c == '\t';
    v->n = tabs + 1 - 9;
    if (v->n < 1 || v->n >= (1ll << 31) || v->nrecords >= (1ll << 31)) return refuse(0, MIH_VCF_HEADER);
    if (v->max_chunk > (1ll << 30)) return refuse(0, MIH_VCF_RAGGED);
    *out = v.release();
    return MIH_OK;
}

int mih_vcf_info(const mih_vcf *v, int64_t *n, int64_t *nrecords, int32_t *container, int64_t *longest_line)
{
    if (!v) { set_error("null argument"); return MIH_BAD_ARG; }
    if (n) *n = v->n;
    if (nrecords) *nrecords = v->nrecords;
    if (container) *container = v->container;
    if (longest_line) *longest_line = v->longest;
    return MIH_OK;
}

static int copy_text(const std::string &s, char *buf, int64_t len, int64_t *need)
{
    if (need) *need = (int64_t)s.size();
    if (buf && len > 0) std::memcpy(buf, s.data(), (size_t)std::min<int64_t>(len, (int64_t)s.size()));
    return MIH_OK;
}

int mih_vcf_header(const mih_vcf *v, char *buf, int64_t len, int64_t *need)
{
    if (!v) { set_error("null argument"); return MIH_BAD_ARG; }
    return copy_text(v->header, buf, len, need);
}

int mih_vcf_meta(const mih_vcf *v, char *buf, int64_t len, int64_t *need)
{
    if (!v) { set_error("null argument"); return MIH_BAD_ARG; }
    return copy_text(v->meta, buf, len, need);
}

int mih_vcf_close(mih_vcf *v)
{
    delete v;
    return MIH_OK;
}

int mih_vcf_inflate(const mih_vcf *v, int threads, int64_t *bytes)
{
    if (!v) { set_error("null argument"); return MIH_BAD_ARG; }
    if (threads < 0) { set_error("threads must be >= 0"); return MIH_BAD_ARG; }
    const int64_t nchunks = (int64_t)v->chunks.size() - 1;
    unsigned nth = v->container == 1 ? 1u : default_workers(threads);
    if ((int64_t)nth > nchunks) nth = (unsigned)std::max<int64_t>(1, nchunks);
    std::atomic<int64_t> next_chunk{0}, total{0};
    std::atomic<int> failed{0};
    auto worker = [&]() {
        ChunkReader rd(v);
        std::vector<uint8_t> txt((size_t)v->max_chunk + 1);
        if (!rd.init()) { failed.store(1); return; }
        for (int64_t c; (c = next_chunk.fetch_add(1)) < nchunks && !failed.load();) {
            if (!rd.fill(c, txt.data())) { failed.store(1); return; }
            total.fetch_add(v->chunks[(size_t)c + 1].off - v->chunks[(size_t)c].off);
        }
    };
    if (nth <= 1) worker();
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nth; ++t) th.emplace_back(worker);
        for (auto &t : th) t.join();
    }
    if (failed.load()) { set_error("%s: cannot be read or inflated as at mih_vcf_open", v->path.c_str()); return MIH_BAD_ARG; }
    if (bytes) *bytes = total.load();
    return MIH_OK;
}

static int vcf_check_args(const mih_vcf *v, int field, int64_t rec0, int64_t nrec, int threads)
{
    if (field != 0 && field != 1) { set_error("field must be 0 (GT) or 1 (DS), got %d", field); return MIH_BAD_ARG; }
    if (rec0 < 0 || nrec <= 0 || rec0 + nrec > v->nrecords) { set_error("records [%lld, %lld) out of range for %lld", (long long)rec0, (long long)(rec0 + nrec), (long long)v->nrecords); return MIH_BAD_DIM; }
    if (threads < 0) { set_error("threads must be >= 0"); return MIH_BAD_ARG; }
    return MIH_OK;
}

// Pass 2.  The tokeniser writes record r of the range into column r - rec0 of the u16 matrix Du (column stride ld), or -- pack
// given -- into a panel of the worker's own that holds the chunk's records, which the pack kernel, queued behind it on the
// worker's stream, turns into those columns of the builder's 2-bit image (a record that is no hard call: MIH_VCF_NOT_HARD_CALL).
// *gcd_out: the gcd of 10^4 and every positive DS numerator.  The caller owns the target and drops it on any failure.
static int vcf_stream(mih_vcf *v, int field, int64_t rec0, int64_t nrec, int threads, int device, uint16_t *Du, int64_t ld,
                      mih_snp_builder *pack, uint32_t *gcd_out, int64_t *bad_record, int32_t *bad_what)
{
    v->meta.clear();
    const int64_t n = v->n, rec1 = rec0 + nrec;
    // the chunks that hold records of the range
    const int64_t nchunks = (int64_t)v->chunks.size() - 1;
    int64_t c_lo = 0, c_hi = nchunks;
    while (c_lo + 1 < nchunks && v->chunks[(size_t)c_lo + 1].rec0 <= rec0) ++c_lo;
    while (c_hi - 1 > c_lo && v->chunks[(size_t)c_hi - 1].rec0 >= rec1) --c_hi;
    const int64_t buf_bytes = round_up(v->max_chunk + 32, 256);     // 16 bytes of slack on either side of a line, for the aligned loads
    const int64_t max_rec = v->max_chunk_records + 1, max_seg = v->max_chunk / kVcfSeg + 2 * max_rec + 2;
    const int64_t desc_bytes = round_up((max_rec + 1) * (int64_t)sizeof(VcfRec), 256);
    unsigned nth = v->container == 1 ? 1u : default_workers(threads);    // a gzip stream has one reader
    if ((int64_t)nth > c_hi - c_lo) nth = (unsigned)(c_hi - c_lo);
    const size_t panel_elems = pack ? (size_t)(max_rec * ld) : 0;         // one worker's panel: the records of the longest chunk
    const size_t staging_budget = 512ull << 20, per_worker = (size_t)(2 * (buf_bytes + desc_bytes));
    const size_t per_worker_dev = per_worker + 2 * sizeof(uint16_t) * panel_elems;
    if (per_worker_dev * nth > staging_budget) nth = (unsigned)std::max<size_t>(1, staging_budget / per_worker_dev);
    int rc = MIH_OK;
    DevBuf<unsigned long long> bad;
    DevBuf<uint32_t> gcdv, segcnt;
    if ((rc = bad.alloc(1)) || (rc = gcdv.alloc(1)) || (rc = segcnt.alloc((size_t)(2 * nth * max_seg)))) return rc;
    const unsigned long long bad0 = ~0ull;
    const uint32_t g0 = 10000u;
    if (hipMemcpy(bad.p, &bad0, sizeof(bad0), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(gcdv.p, &g0, sizeof(g0), hipMemcpyHostToDevice) != hipSuccess) return MIH_HIP_ERROR;
    struct Staging {
        uint8_t *pin = nullptr, *dev = nullptr;
        ~Staging() { if (pin) (void)hipHostFree(pin); if (dev) (void)hipFree(dev); }
    } stg;
    for (;;) {                         // a failed allocation degrades to one worker before it fails the create
        if (hipHostMalloc((void **)&stg.pin, per_worker * nth, hipHostMallocDefault) == hipSuccess &&
            device_malloc((void **)&stg.dev, per_worker * nth) == hipSuccess) break;
        (void)hipGetLastError();
        if (stg.pin) { (void)hipHostFree(stg.pin); stg.pin = nullptr; }
        if (stg.dev) { (void)hipFree(stg.dev); stg.dev = nullptr; }
        if (nth == 1) { set_error("allocation of the VCF staging buffers (%zu bytes pinned + device) failed", per_worker); return MIH_OOM; }
        nth = 1;
    }
    DevBuf<uint16_t> panels;
    if (pack && (rc = panels.alloc(2 * nth * panel_elems))) return rc;

    std::atomic<unsigned long long> host_bad{~0ull};               // (record << 8) | reason, the least
    auto flag = [&](int64_t record, int what) {
        const unsigned long long key = ((unsigned long long)record << 8) | (unsigned long long)what;
        unsigned long long cur = host_bad.load();
        while (key < cur && !host_bad.compare_exchange_weak(cur, key)) {}
    };
    std::mutex mu;
    std::string err_msg;
    std::atomic<int> failed{0};
    std::vector<std::string> metas((size_t)nchunks);
    std::atomic<int64_t> next_chunk{v->container == 1 ? 0 : c_lo};
    std::atomic<unsigned> worker_no{0};
    const char *key = field ? "DS" : "GT";
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
        auto unreadable = [&](int64_t c) { flag(std::max(rec0, v->chunks[(size_t)c].rec0), MIH_VCF_IO); };   // the file changed since pass 1
        auto broken = [&](const char *what) { std::lock_guard<std::mutex> g(mu); if (err_msg.empty()) err_msg = what; failed.store(1); };
        if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&r.st) != hipSuccess) return broken("VCF worker: stream");
        for (int i = 0; i < 2; ++i)
            if (hipEventCreateWithFlags(&r.done[i], hipEventDisableTiming) != hipSuccess) return broken("VCF worker: event");
        ChunkReader rd(v);
        if (!rd.init()) return broken("VCF worker: zlib");
        for (int64_t it = 0;; ++it) {
            const int64_t c = next_chunk.fetch_add(1);
            if (c >= c_hi || failed.load()) break;
            if ((int64_t)(host_bad.load() >> 8) < v->chunks[(size_t)c].rec0) break;      // a bad record before this chunk
            const int64_t len = v->chunks[(size_t)c + 1].off - v->chunks[(size_t)c].off;
            const int b = (int)(it & 1);
            uint8_t *pin = stg.pin + per_worker * me + (size_t)b * (size_t)(buf_bytes + desc_bytes);
            uint8_t *dev = stg.dev + per_worker * me + (size_t)b * (size_t)(buf_bytes + desc_bytes);
            uint8_t *txt = pin + 16;                                // the chunk's text
            VcfRec *desc = reinterpret_cast<VcfRec *>(pin + buf_bytes);
            if (it >= 2 && hipEventSynchronize(r.done[b]) != hipSuccess) return broken("VCF worker: kernel failed");
            if (!rd.fill(c, txt)) return unreadable(c);
            if (c < c_lo) { --it; continue; }                      // gzip: text before the range, inflated and dropped
            // ---- the records of the chunk: nine fields on the host, the rest described for the device
            int64_t rec = v->chunks[(size_t)c].rec0, nd = 0;
            const int64_t rec_first = std::max(rec, rec0);          // a panel's column 0
            const int64_t col_base = pack ? rec_first : rec0;
            uint32_t seg = 0;
            std::string &meta = metas[(size_t)c];
            for (int64_t p = 0; p < len;) {
                const uint8_t *nl = (const uint8_t *)memchr(txt + p, '\n', (size_t)(len - p));
                const int64_t le = nl ? nl - txt : len;
                if (le == p || txt[p] != '#') {
                    if (rec >= rec0 && rec < rec1) {
                        int64_t tab[9], q = p;
                        int nt = 0;
                        for (; nt < 9; ++nt) {
                            const uint8_t *t = (const uint8_t *)memchr(txt + q, '\t', (size_t)(le - q));
                            if (!t) break;
                            tab[nt] = t - txt; q = tab[nt] + 1;
                        }
                        int what = 0, k = -1;
                        if (nt < 9) what = MIH_VCF_RAGGED;
                        else {
                            for (int64_t i = p; i < tab[8]; ++i) if (txt[i] == '\r' || txt[i] >= 0x80) what = MIH_VCF_TOKEN;
                            if (tab[1] - tab[0] - 1 < 1 || tab[1] - tab[0] - 1 > 18) what = MIH_VCF_TOKEN;       // POS: digits only
                            for (int64_t i = tab[0] + 1; i < tab[1]; ++i) if (txt[i] < '0' || txt[i] > '9') what = MIH_VCF_TOKEN;
                            if (!what && memchr(txt + tab[3] + 1, ',', (size_t)(tab[4] - tab[3] - 1))) what = MIH_VCF_MULTIALLELIC;
                            int sub = 0;
                            for (int64_t i = tab[7] + 1; i < tab[8] && k < 0;) {         // the first FORMAT subfield that is the key
                                int64_t e = i;
                                while (e < tab[8] && txt[e] != ':') ++e;
                                if (e - i == 2 && txt[i] == key[0] && txt[i + 1] == key[1]) k = sub;
                                i = e + 1; ++sub;
                            }
                            if (!what && k < 0) what = MIH_VCF_NOKEY;
                        }
                        if (what) { flag(rec, what); break; }
                        desc[nd++] = {(uint32_t)(16 + tab[8] + 1), (uint32_t)(16 + le), k, (int32_t)(rec - col_base), seg};
                        const uint32_t a0 = (uint32_t)(16 + tab[8] + 1) & ~15u;
                        seg += std::max<uint32_t>(1u, (uint32_t)((16 + le - a0 + kVcfSeg - 1) / kVcfSeg));
                        meta.append((const char *)txt + p, (size_t)(tab[4] - p));
                        meta.push_back('\n');
                    }
                    ++rec;
                }
                p = le + 1;
            }
            if (nd > 0) {
                desc[nd] = {0u, 0u, 0, 0, seg};                    // the sentinel: where the last record's segments end
                uint32_t *cnt = segcnt.p + (size_t)(2 * me + b) * (size_t)max_seg;
                const VcfRec *ddesc = reinterpret_cast<const VcfRec *>(dev + buf_bytes);
                if (hipMemcpyAsync(dev, pin, (size_t)round_up(16 + len + 16, 16), hipMemcpyHostToDevice, r.st) != hipSuccess ||
                    hipMemcpyAsync(dev + buf_bytes, desc, (size_t)(nd + 1) * sizeof(VcfRec), hipMemcpyHostToDevice, r.st) != hipSuccess)
                    return broken("VCF worker: H2D copy");
                uint16_t *dst = pack ? panels.p + (size_t)(2 * me + b) * panel_elems : Du;
                hipLaunchKernelGGL(k_vcf_count, dim3(seg), dim3(256), 0, r.st, dev, ddesc, (int)nd, col_base, cnt, bad.p);
                if (field) hipLaunchKernelGGL(k_vcf_parse<1>, dim3(seg), dim3(256), 0, r.st, dev, ddesc, (int)nd, col_base, cnt, n, dst, ld, bad.p, gcdv.p);
                else hipLaunchKernelGGL(k_vcf_parse<0>, dim3(seg), dim3(256), 0, r.st, dev, ddesc, (int)nd, col_base, cnt, n, dst, ld, bad.p, gcdv.p);
                // DS numerators are over 10^4 here (no gcd has been taken), GT counts over 1
                if (pack && snp_builder_pack(pack, rec_first - rec0, nd, dst, ld, field ? 10000u : 1u, bad.p, (unsigned long long)rec_first, 8,
                                             MIH_VCF_NOT_HARD_CALL, r.st) != MIH_OK) return broken("VCF worker: pack");
            }
            if (hipEventRecord(r.done[b], r.st) != hipSuccess) return broken("VCF worker: event record");
        }
        if (hipStreamSynchronize(r.st) != hipSuccess) return broken("VCF tokeniser kernel failed");
    };
    if (nth <= 1) worker();
    else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nth; ++t) th.emplace_back(worker);
        for (auto &t : th) t.join();
    }
    if (failed.load()) { set_error("%s", err_msg.c_str()); (void)hipGetLastError(); return MIH_HIP_ERROR; }

    unsigned long long dev_bad = ~0ull;
    uint32_t g = 10000u;
    if (hipMemcpy(&dev_bad, bad.p, sizeof(dev_bad), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&g, gcdv.p, sizeof(g), hipMemcpyDeviceToHost) != hipSuccess) return MIH_HIP_ERROR;
    const unsigned long long first = std::min(dev_bad, host_bad.load());
    if (first != ~0ull) {
        *bad_record = (int64_t)(first >> 8); *bad_what = (int32_t)(first & 0xFF);
        set_error("%s: record %lld: %s", v->path.c_str(), (long long)(*bad_record + 1), vcf_reason(*bad_what));
        return MIH_BAD_ARG;
    }
    for (int64_t c = c_lo; c < c_hi; ++c) v->meta += metas[(size_t)c];
    *gcd_out = g;
    return MIH_OK;
}

int mih_dosage_create_vcf(mih_vcf *v, int field, int64_t rec0, int64_t nrec, int threads, int device, mih_mat **out,
                          int32_t *denom_out, int64_t *bad_record, int32_t *bad_what)
{
    if (!v || !out || !denom_out || !bad_record || !bad_what) { set_error("null argument"); return MIH_BAD_ARG; }
    *out = nullptr; *bad_record = -1; *bad_what = 0;
    MIH_TRY(vcf_check_args(v, field, rec0, nrec, threads));
    MIH_TRY(select_device(device));
    mih_mat *h = new mih_mat();
    auto fail = [&](int code) { mih_mat_destroy(h); return code; };
    int rc = dosage_alloc(h, v->n, nrec, 1, device);
    if (rc) return fail(rc);
    uint32_t g = 10000u;
    if ((rc = vcf_stream(v, field, rec0, nrec, threads, device, h->Du, h->du_ld, nullptr, &g, bad_record, bad_what))) return fail(rc);
    if (field && g > 1u) hipLaunchKernelGGL(k_vcf_reduce, dim3((unsigned)h->p), dim3(256), 0, h->stream, h->Du, h->du_ld, g);
    h->denom = field ? (int32_t)(10000u / g) : 1;
    if ((rc = dosage_stats(h))) return fail(rc);
    *denom_out = h->denom;
    *out = h;
    return MIH_OK;
}

int mih_snp_create_vcf(mih_vcf *v, int field, int64_t rec0, int64_t nrec, int threads, int center, int scale, int impute, int dtype,
                       int device, mih_mat **out, int64_t *bad_record, int32_t *bad_what)
{
    if (!v || !out || !bad_record || !bad_what) { set_error("null argument"); return MIH_BAD_ARG; }
    *out = nullptr; *bad_record = -1; *bad_what = 0;
    MIH_TRY(vcf_check_args(v, field, rec0, nrec, threads));
    mih_snp_builder *b = nullptr;
    MIH_TRY(mih_snp_builder_create(v->n, nrec, center, scale, impute, dtype, device, &b));
    uint32_t g = 10000u;
    int rc = vcf_stream(v, field, rec0, nrec, threads, device, nullptr, round_up(v->n, 8), b, &g, bad_record, bad_what);
    if (!rc) {
        snp_builder_cover_all(b);
        rc = mih_snp_builder_finish(b, out);
    }
    mih_snp_builder_destroy(b);
    return rc;
}

}  // extern "C"
