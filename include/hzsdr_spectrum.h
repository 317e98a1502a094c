/*
 * hzsdr_spectrum.h -- the fused power spectrum of libhzsdr_hip: windowed
 * forward transforms of (overlapping) frames of an IQ stream, |X|^2, averaged
 * over `avg` frames per output row, in one pass over the raw samples.
 *
 * The entries live beside hzsdr.h (same conventions, same status codes, same
 * context) until the Go binding takes them up.  Each declaration cites the
 * reference interface (file:line under the go-sdr checkout) it relates to.
 *
 * Definitions (stream positions count from the first sample pushed since
 * create or reset; K = avg):
 *   - frame j covers samples [j*hop, j*hop + n); each sample is converted as
 *     hzsdr_convert converts it, then multiplied by w[i] (one float32 multiply
 *     per component; window == NULL is rectangular);
 *   - p_j[k] = |X_j[k]|^2 in float32, X_j the forward transform (the sign
 *     convention of fft.Forward, fft/fft.go:32-35);
 *   - row r: P_r[k] = scale * (((+0 + p_{rK}[k]) + p_{rK+1}[k]) + ... + p_{rK+K-1}[k]),
 *     summed in float32 in frame order; HZSDR_SPECTRUM_DB writes
 *     10*log10(P_r[k]) in float32 (-inf where P_r[k] == 0);
 *   - HZSDR_ORDER_NEGATIVE_FIRST rows are the ZERO_FIRST rows with their
 *     halves swapped (FrequencySlice.Shift, fft/result.go:82-97).
 * Because the order of every sum is fixed, the output does not depend on how
 * the stream is cut into pushes, on the kernel form, or on the memory space.
 */
#ifndef HZSDR_SPECTRUM_H
#define HZSDR_SPECTRUM_H

#include "hzsdr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hzsdr_spectrum hzsdr_spectrum;

/* fft.Order, fft/result.go:34-47: ZeroFirst = false, NegativeFirst = true */
#define HZSDR_ORDER_ZERO_FIRST 0
#define HZSDR_ORDER_NEGATIVE_FIRST 1

/* output kind */
#define HZSDR_SPECTRUM_POWER 0
#define HZSDR_SPECTRUM_DB 1

/* kernel forms (hzsdr_spectrum_options / hzsdr_spectrum_last_form) */
#define HZSDR_SPECTRUM_FORM_AUTO 0
#define HZSDR_SPECTRUM_FORM_ROW_WALK 1
#define HZSDR_SPECTRUM_FORM_FRAME_PARALLEL 2

/* A spectrum of src_format samples (iq.go:110-126) with n-point transforms
 * (fft.Planner, fft/fft.go:42-48; n a power of two, 256 .. 8192), frames `hop`
 * samples apart (hop > n skips samples), `avg` frames per row.  `window`: n
 * float32 host values, or NULL.  `order`: HZSDR_ORDER_*; `output`:
 * HZSDR_SPECTRUM_POWER or _DB.  The transform's tables are prepared here.
 * HZSDR_ERR_INVALID_ARGUMENT for n outside the range, hop == 0, avg == 0, a bad
 * order or output kind; HZSDR_ERR_FORMAT_UNKNOWN for an unknown format. */
int hzsdr_spectrum_create(hzsdr_ctx *ctx, int src_format, size_t n, size_t hop, size_t avg,
                          const float *window, float scale, int order, int output,
                          hzsdr_spectrum **out);
/* Consume n_in samples of `in` (all of them) and write every row that
 * completes during the push to `out` (rows x n float32, row-major; the bins of
 * a FrequencySlice, fft/result.go:49-63, as power).  The unfinished frame, the
 * samples still to skip and the partial row stay on the device for the next
 * push.  HZSDR_ERR_DST_TOO_SMALL when out_rows_cap is below the rows the push
 * completes: checked before anything is launched; the state is unchanged.
 * Stream-ordered on the context's stream; HOST contexts stage `in` and `out`. */
int hzsdr_spectrum_push(hzsdr_spectrum *s, const void *in, size_t n_in, float *out, size_t out_rows_cap,
                        size_t *rows_written);
/* The rows a push of n_in samples would write now. */
int hzsdr_spectrum_rows_for(const hzsdr_spectrum *s, size_t n_in, size_t *rows);
/* Frames already summed into the unfinished row, and samples held for the
 * next frame. */
int hzsdr_spectrum_pending(const hzsdr_spectrum *s, size_t *frames_in_row, size_t *samples_held);
/* Kernel form of later pushes: HZSDR_SPECTRUM_FORM_AUTO (default), _ROW_WALK
 * or _FRAME_PARALLEL.  Every form writes the same bits. */
int hzsdr_spectrum_options(hzsdr_spectrum *s, int form);
/* The form the last push with frames ran (0 before any). */
int hzsdr_spectrum_last_form(const hzsdr_spectrum *s, int *form);
/* Back to stream position 0: no samples held, no partial row. */
int hzsdr_spectrum_reset(hzsdr_spectrum *s);
int hzsdr_spectrum_free(hzsdr_spectrum *s);

#ifdef __cplusplus
}
#endif

#endif /* HZSDR_SPECTRUM_H */
