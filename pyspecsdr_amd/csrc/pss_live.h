// pss_live.h — the host side of the dead-read rule and of the streamed loop's bookkeeping (include/pss.h, "replaying a capture"): plain C++,
// no HIP, no context, so that it also compiles into a stand-alone program.
//
// Reference: the main loop drops a read buffer before anything else looks at it,
//     if len(samples) == 0 or np.all(samples == 0): ...; continue                                   (pyspecsdr.py:2237)
// read_samples hands the driver a zero-filled array (:1887), so a read that timed out comes back all zero.
#pragma once
#include <cstdint>
#include <cstring>

namespace pss_live {

// NumPy's `== 0` on a float32 word, decided on the bits: +0.0 and -0.0 are zero, a NaN and the smallest denormal are not.  No float compare:
// the answer must not depend on a denormal mode.
inline bool word_is_zero(uint32_t bits) { return (bits & 0x7fffffffu) == 0; }

// live[f] = !np.all(frame_f == 0) over frames of 2 n float32 words; the live frames' indices in ascending order; returns their number.
// live and live_idx may be null; entries of live_idx behind the count stay untouched.
inline long live_frames(const float *iq, long n_frames, int n, uint8_t *live, int32_t *live_idx)
{
    const size_t words = 2 * (size_t)n;
    long count = 0;
    for (long f = 0; f < n_frames; f++) {
        const unsigned char *p = reinterpret_cast<const unsigned char *>(iq) + (size_t)f * words * sizeof(uint32_t);
        bool any = false;
        for (size_t w = 0; w < words && !any; w++) {
            uint32_t bits;
            memcpy(&bits, p + w * sizeof(uint32_t), sizeof bits);
            any = !word_is_zero(bits);
        }
        if (live) live[f] = any ? 1 : 0;
        if (any && live_idx) live_idx[count] = (int32_t)f;
        count += any;
    }
    return count;
}

// Where the streamed loop stands between two chunks: how many live / open frames lie behind it (the offsets of the next downloads) and the
// squelch gate's state.  Dead frames advance nothing: the reference's `continue` precedes the gate, the history and ui_update_counter.
struct Cursor {
    long n_live = 0, n_open = 0;
    double held = 0.0;
    int phase = 0;
    void advance(long live, long open, double held_out, int every)
    {
        n_live += live;
        n_open += open;
        held = held_out;
        if (every > 0) phase = (int)(((long)phase + live) % every);
    }
};

}  // namespace pss_live
