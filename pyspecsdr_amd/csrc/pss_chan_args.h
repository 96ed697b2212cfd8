// pss_chan_args.h — the argument rules the channelisers share (pss_pfb / pss_h_pfb, pss_bank / pss_h_bank), stated once: the two calls
// differ in which channel counts they take and in the name their reasons carry, and in nothing else.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>

#include "pss_ctx.h"
#include "pss_pfb.h"

// ctx: where the reason goes (NULL: the library's own slot).  who: the call's name, the prefix of every reason.  chan_ok: whether the call
// takes n_chan; chan_why: the reason where it does not.
inline int pss_chan_args_check(pss_ctx *ctx, const char *who, bool chan_ok, const char *chan_why, const void *iq, long n_buf, long buf_index0,
                               long n_capture, int n_chan, int decim, const double *taps, int n_taps, int lead, long m_begin, long m_end, const void *out,
                               long out_stride)
{
    auto bad = [&](const char *why) { return pss_fail(ctx, PSS_E_ARG, std::string(who) + ": " + why); };
    if (!chan_ok) return bad(chan_why);
    if (decim < 1 || decim > n_chan) return bad("decim outside [1, n_chan]");
    if (n_taps < 1 || n_taps > pss_pf::TAPS_PER_CHAN * n_chan) return bad("n_taps outside [1, 32 n_chan]");
    if (!taps) return bad("null taps");
    if (lead < 0 || lead > n_taps - 1) return bad("lead outside [0, n_taps - 1]");
    for (int k = 0; k < n_taps; k++)
        if (!std::isfinite(taps[k])) return bad("a tap that is not finite");
    if (n_capture < 0 || n_buf < 0 || buf_index0 < 0 || n_buf > n_capture || buf_index0 > n_capture - n_buf)
        return bad("the buffer [buf_index0, buf_index0 + n_buf) is not inside the capture [0, n_capture)");
    if (m_begin < 0 || m_end < m_begin || m_end > pss_dc::out_len(n_capture, decim)) return bad("[m_begin, m_end) outside [0, ceil(n_capture / decim)]");
    if (out_stride < m_end - m_begin) return bad("out_stride < m_end - m_begin");
    if ((reinterpret_cast<uintptr_t>(iq) & 7) || (reinterpret_cast<uintptr_t>(out) & 7)) return bad("the input and the output must be 8-byte aligned");
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
