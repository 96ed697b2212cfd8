// pss_bars.h — the spectrum display (draw_spectrogram, pyspecsdr.py:399-499) in its compact per-column form.  Every cell the reference
// draws in a column follows from two small integers: the bar's height in cells, min(int(value * disp_h), disp_h) (:458), and the level of
// `value` against the thresholds 0.8 / 0.4 / 0.2 (:476-491).  One rule, for the device (k_spectrogram, k_bars_cells) and for the host
// (pss_h_bars_cells: a curses front end draws from the 2 x disp_w bytes it downloaded).
#pragma once
#include <hip/hip_runtime.h>

namespace pss_bars {

// cell (y, column) of the grid from the column's bar.  glyph 0 '.', 1 '-', 2 '=', 3 '#', 4 ' '; colour: the curses pair (1 = cleared
// cell above the bar); height < 0: the column is not drawn (-1, -1).
__host__ __device__ inline void cell(int height, int level, int disp_h, int y, int &glyph, int &colour)
{
    if (height < 0) { glyph = -1; colour = -1; return; }
    glyph = 4;
    colour = 1;
    if (y < disp_h - height) return;
    const double rel = height > 0 ? (double)(y - (disp_h - height)) / (double)height : 0.0;   // (:473)
    if (level >= 3) { glyph = rel > 0.5 ? 3 : 2; colour = 14; }
    else if (level == 2) { glyph = rel > 0.5 ? 2 : 1; colour = 13; }
    else if (level == 1) { glyph = rel > 0.5 ? 1 : 0; colour = 12; }
    else if (rel > 0.7) { glyph = 0; colour = 11; }
    else { glyph = 4; colour = 10; }
}

}  // namespace pss_bars
