// pss_chan.h — what the units of the channel family share around their arithmetic headers, stated once: the capture-window rules of
// pss_ddc / pss_pfb / pss_bank and their host twins, the channelisers' argument rules, the rotor knots on the host and the host twins'
// loop over output instants.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "pss_ctx.h"
#include "pss_pfb.h"

// pss_dc::build_knots' table on the host: what pss_ddc and pss_pfb upload and what their host twins read
inline const double *pss_host_knots()
{
    static const std::vector<double> k = [] {
        std::vector<double> v(2 * pss_dc::KNOTS);
        pss_dc::build_knots(v.data());
        return v;
    }();
    return k.data();
}

// The rules of a window [m_begin, m_end) of outputs at fs / decim over a buffer that holds [buf_index0, buf_index0 + n_buf) of a capture,
// behind the caller's own rules for decim, n_taps and the null test of taps.  ctx: where the reason goes (NULL: the library's own slot).
// who: the call's name, the prefix of every reason.  align8: iq and out must be 8-byte aligned, tested before the empty window returns
// (the channelisers; pss_ddc tests its device pointers itself behind this check, pss_h_ddc takes any pointer).
inline int pss_chan_window_check(pss_ctx *ctx, const char *who, bool align8, const void *iq, long n_buf, long buf_index0, long n_capture, int decim,
                                 const double *taps, int n_taps, int lead, long m_begin, long m_end, const void *out, long out_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (lead < 0 || lead > n_taps - 1) return bad("lead outside [0, n_taps - 1]");
    for (int k = 0; k < n_taps; k++)
        if (!std::isfinite(taps[k])) return bad("a tap that is not finite");
    if (n_capture < 0 || n_buf < 0 || buf_index0 < 0 || n_buf > n_capture || buf_index0 > n_capture - n_buf)
        return bad("the buffer [buf_index0, buf_index0 + n_buf) is not inside the capture [0, n_capture)");
    if (m_begin < 0 || m_end < m_begin || m_end > pss_dc::out_len(n_capture, decim)) return bad("[m_begin, m_end) outside [0, ceil(n_capture / decim)]");
    if (out_stride < m_end - m_begin) return bad("out_stride < m_end - m_begin");
    if (align8 && ((reinterpret_cast<uintptr_t>(iq) & 7) || (reinterpret_cast<uintptr_t>(out) & 7)))
        return bad("the input and the output must be 8-byte aligned");
    if (m_begin == m_end) return PSS_OK;
    if (!out) return bad("null output");
    // the samples the outputs need, cut to the capture: they must lie in the buffer
    long need_lo = m_begin * decim + lead - (n_taps - 1), need_hi = (m_end - 1) * decim + lead + 1;
    if (need_lo < 0) need_lo = 0;
    if (need_hi > n_capture) need_hi = n_capture;
    if (need_lo < need_hi) {
        if (!iq) return bad("null input");
        if (need_lo < buf_index0 || need_hi > buf_index0 + n_buf) return bad("an output needs a sample of the capture that the buffer does not hold");
    }
    return PSS_OK;
}

// The argument rules the channelisers share (pss_pfb / pss_h_pfb, pss_bank / pss_h_bank): the two calls differ in which channel counts they
// take and in the name their reasons carry, and in nothing else.  chan_ok: whether the call takes n_chan; chan_why: the reason where it
// does not.
inline int pss_chan_args_check(pss_ctx *ctx, const char *who, bool chan_ok, const char *chan_why, const void *iq, long n_buf, long buf_index0,
                               long n_capture, int n_chan, int decim, const double *taps, int n_taps, int lead, long m_begin, long m_end, const void *out,
                               long out_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (!chan_ok) return bad(chan_why);
    if (decim < 1 || decim > n_chan) return bad("decim outside [1, n_chan]");
    if (n_taps < 1 || n_taps > pss_pf::TAPS_PER_CHAN * n_chan) return bad("n_taps outside [1, 32 n_chan]");
    if (!taps) return bad("null taps");
    return pss_chan_window_check(ctx, who, true, iq, n_buf, buf_index0, n_capture, decim, taps, n_taps, lead, m_begin, m_end, out, out_stride);
}

// The host twins' loop (pss_h_pfb, pss_h_bank): the instants m_begin .. m_end - 1 one by one, each M channels from
// instant(m, X, vr, vi, y) — X(j, xr, xi) hands out capture sample j, zero outside the buffer [buf_index0, buf_index0 + n_buf) — scattered
// to h_out[channel][instant].
template <class FI>
void pss_chan_host_loop(const float *h_iq, long n_buf, long buf_index0, int n_chan, long m_begin, long m_end, float *h_out, long out_stride, FI instant)
{
    const long lo = buf_index0, hi = buf_index0 + n_buf;
    std::vector<double> vr(n_chan), vi(n_chan);
    std::vector<float> y(2 * (size_t)n_chan);
    for (long m = m_begin; m < m_end; m++) {
        instant(m, [&](long j, float &xr, float &xi) {
            const bool in = j >= lo && j < hi;
            xr = in ? h_iq[2 * (j - lo)] : 0.0f;
            xi = in ? h_iq[2 * (j - lo) + 1] : 0.0f;
        }, vr.data(), vi.data(), y.data());
        for (int c = 0; c < n_chan; c++) {
            float *o = h_out + 2 * ((size_t)c * out_stride + (m - m_begin));
            o[0] = y[2 * c];
            o[1] = y[2 * c + 1];
        }
    }
}
