// profile.hip -- per-launch HIP-event timing of the dominant kernel, on the matrix handle (mih_profile_*; bench.py roofline)
#include "common.h"

namespace mih {

bool prof_begin(const mih_mat *h, hipStream_t s, PassRecord &rec)
{
    Profile &pf = *h->prof;
    if (!pf.on) return false;
    if (hipEventCreate(&rec.e0) != hipSuccess || hipEventCreate(&rec.e1) != hipSuccess) { rec.e0 = rec.e1 = nullptr; (void)hipGetLastError(); return false; }
    (void)hipEventRecord(rec.e0, s);
    return true;
}
void prof_end(const mih_mat *h, hipStream_t s, PassRecord &rec)
{
    (void)hipEventRecord(rec.e1, s);
    Profile &pf = *h->prof;
    std::lock_guard<std::mutex> g(pf.mu);
    pf.open.push_back(rec);
}
void Profile::drain()
{
    for (auto &r : open) {
        float ms = 0.f, st = 0.f;
        mih_pass_record out;
        memset(&out, 0, sizeof(out));
        if (hipEventSynchronize(r.e1) == hipSuccess && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) {
            if (origin && hipEventElapsedTime(&st, origin, r.e0) != hipSuccess) { st = 0.f; (void)hipGetLastError(); }
            out.start_ms = st; out.ms = ms; out.residuals = r.residuals; out.operands = r.operands; out.stream_tag = r.stream_tag;
            memcpy(out.kernel, r.kernel, sizeof(out.kernel));
            done.push_back(out);
        } else (void)hipGetLastError();
        (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    }
    open.clear();
}
Profile::~Profile()
{
    for (auto &r : open) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (auto &r : xopen) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    if (origin) (void)hipEventDestroy(origin);
}

}  // namespace mih

using namespace mih;

extern "C" {

int mih_profile_enable(const mih_mat *h, int on)
{
    if (!h) { set_error("null matrix handle"); return MIH_BAD_ARG; }
    Profile &pf = *h->prof;
    std::lock_guard<std::mutex> g(pf.mu);
    if (on && !pf.on) {
        MIH_HIP(hipSetDevice(h->device));
        if (pf.origin) { (void)hipEventDestroy(pf.origin); pf.origin = nullptr; }
        MIH_HIP(hipEventCreate(&pf.origin));
        MIH_HIP(hipEventRecord(pf.origin, h->stream));
    }
    pf.on = on != 0;
    return MIH_OK;
}

int mih_profile_read(const mih_mat *h, double *xtv_kernel_ms, int64_t *xtv_launches, int reset)
{
    if (!h) { set_error("null matrix handle"); return MIH_BAD_ARG; }
    Profile &pf = *h->prof;
    std::lock_guard<std::mutex> g(pf.mu);
    pf.drain();
    double ms = 0.0;
    for (const auto &r : pf.done) ms += r.ms;
    if (xtv_kernel_ms) *xtv_kernel_ms = ms;
    if (xtv_launches) *xtv_launches = (int64_t)pf.done.size();
    if (reset) pf.done.clear();
    return MIH_OK;
}

int mih_profile_passes(const mih_mat *h, mih_pass_record *out, int64_t cap, int64_t *n, int reset)
{
    if (!h || !n) { set_error("null argument"); return MIH_BAD_ARG; }
    Profile &pf = *h->prof;
    std::lock_guard<std::mutex> g(pf.mu);
    pf.drain();
    *n = (int64_t)pf.done.size();
    if (out) for (int64_t i = 0; i < cap && i < *n; ++i) out[i] = pf.done[(size_t)i];
    if (reset) pf.done.clear();
    return MIH_OK;
}

int mih_profile_exchange(const mih_mat *h, double *ms4, int64_t *count4, int reset)
{
    if (!h || !ms4 || !count4) { set_error("null argument"); return MIH_BAD_ARG; }
    Profile &pf = *h->prof;
    std::lock_guard<std::mutex> g(pf.mu);
    for (auto &r : pf.xopen) {
        float ms = 0.f;
        if (hipEventSynchronize(r.e1) == hipSuccess && hipEventElapsedTime(&ms, r.e0, r.e1) == hipSuccess) { pf.xms[r.kind] += ms; ++pf.xcount[r.kind]; }
        else (void)hipGetLastError();
        (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1);
    }
    pf.xopen.clear();
    for (int i = 0; i < 4; ++i) { ms4[i] = pf.xms[i]; count4[i] = pf.xcount[i]; if (reset) { pf.xms[i] = 0.0; pf.xcount[i] = 0; } }
    return MIH_OK;
}

int mih_profile_counters(const mih_mat *h, int64_t *out, int reset)
{
    if (!h || !out) { set_error("null argument"); return MIH_BAD_ARG; }
    Profile &pf = *h->prof;
    std::lock_guard<std::mutex> g(pf.mu);
    for (int i = 0; i < MIH_PROFILE_NCOUNTERS; ++i) { out[i] = pf.counters[i]; if (reset) pf.counters[i] = 0; }
    return MIH_OK;
}

}  // extern "C"
