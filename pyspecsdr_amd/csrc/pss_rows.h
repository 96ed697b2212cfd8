// pss_rows.h — the row type chooses the entry point: float rows go to pss_X, double rows to pss_X_f64.  Host-side forwarders for the code that
// runs rows of either type through one schedule (pss_pipeline.hip: frame_pipeline<TR>, pss_stream.cpp: stream_display<TR>).
#pragma once
#include "pss_ctx.h"

namespace pss_rows {
inline int spectrum_db(pss_ctx *c, const float *iq, long nf, int n, float *db) { return pss_spectrum_db(c, iq, nf, n, db); }
inline int spectrum_db(pss_ctx *c, const float *iq, long nf, int n, double *db) { return pss_spectrum_db_f64(c, iq, nf, n, db); }
// smoothing + median clamp, and the extremes of every post-processed row
inline int post(pss_ctx *c, const float *db, long nf, int n, float *post, float *lo, float *hi) { return pss_spectrum_post_extremes(c, db, nf, n, post, lo, hi); }
inline int post(pss_ctx *c, const double *db, long nf, int n, double *post, double *lo, double *hi) { return pss_spectrum_post_f64(c, db, nf, n, post, lo, hi); }
// the newest line of every frame (len = n - 4 points a row, h rows of halo in front of lo / hi, history w)
inline int waterfall_rows(pss_ctx *c, const float *p, long nf, int len, const float *lo, const float *hi, int h, int w, int dw, int8_t *a, int8_t *b) { return pss_waterfall_rows(c, p, nf, len, lo, hi, h, w, dw, a, b); }
inline int waterfall_rows(pss_ctx *c, const double *p, long nf, int len, const double *lo, const double *hi, int h, int w, int dw, int8_t *a, int8_t *b) { return pss_waterfall_rows_f64(c, p, nf, len, lo, hi, h, w, dw, a, b); }
inline int persistence_rows(pss_ctx *c, const float *p, long nf, int len, const float *lo, const float *hi, int h, int w, int dh, int dw, int8_t *a) { return pss_persistence_rows(c, p, nf, len, lo, hi, h, w, dh, dw, a); }
inline int persistence_rows(pss_ctx *c, const double *p, long nf, int len, const double *lo, const double *hi, int h, int w, int dh, int dw, int8_t *a) { return pss_persistence_rows_f64(c, p, nf, len, lo, hi, h, w, dh, dw, a); }
inline int gradient_rows(pss_ctx *c, const float *p, long nf, int len, const float *lo, const float *hi, int h, int w, int dw, int8_t *a, int8_t *b) { return pss_gradient_rows(c, p, nf, len, lo, hi, h, w, dw, a, b); }
inline int gradient_rows(pss_ctx *c, const double *p, long nf, int len, const double *lo, const double *hi, int h, int w, int dw, int8_t *a, int8_t *b) { return pss_gradient_rows_f64(c, p, nf, len, lo, hi, h, w, dw, a, b); }
// the whole screen from the rows of a history
inline int waterfall_cells(pss_ctx *c, const float *r, int nr, int len, int dh, int dw, int8_t *a, int8_t *b) { return pss_waterfall_cells(c, r, nr, len, dh, dw, a, b); }
inline int waterfall_cells(pss_ctx *c, const double *r, int nr, int len, int dh, int dw, int8_t *a, int8_t *b) { return pss_waterfall_cells_f64(c, r, nr, len, dh, dw, a, b); }
inline int persistence_cells(pss_ctx *c, const float *r, int nr, int len, int dh, int dw, int8_t *a) { return pss_persistence_cells(c, r, nr, len, dh, dw, a); }
inline int persistence_cells(pss_ctx *c, const double *r, int nr, int len, int dh, int dw, int8_t *a) { return pss_persistence_cells_f64(c, r, nr, len, dh, dw, a); }
// the display chain without materialised post-processed rows (pss_ctx.h: pss_chain_vals_*)
inline int chain_vals(pss_ctx *c, const float *db, long nf, int n, float *lo, float *hi, int h, int w, int display, int dh, int dw, int8_t *a, int8_t *b, double *vals)
{
    return pss_chain_vals_f32(c, db, nf, n, lo, hi, h, w, display, dh, dw, a, b, vals);
}
inline int chain_vals(pss_ctx *c, const double *db, long nf, int n, double *lo, double *hi, int h, int w, int display, int dh, int dw, int8_t *a, int8_t *b, double *vals)
{
    return pss_chain_vals_f64(c, db, nf, n, lo, hi, h, w, display, dh, dw, a, b, vals);
}
}  // namespace pss_rows
