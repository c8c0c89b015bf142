/*
 * wfhip.h — C ABI of libwfhip.so: the MI355X (gfx950) kernels behind the
 * `waveforms.cpm` / `waveforms.filters` / `waveforms.viterbi` / `waveforms.glfsr` /
 * `waveforms.noise` Python API of mcdiarmid/waveforms.
 *
 * The reference has no FFI of its own (it is pure Python + NumPy); the boundary
 * is its Python module API.  Each entry point below replaces the NumPy / Python
 * loop at the cited reference location (paths relative to the reference repo)
 * and is bound from Python with ctypes (waveforms_amd/_hip.py; binding stub in
 * INTEGRATION.md).
 *
 * Conventions
 *  - plain pointers and sizes only; every `d_*` pointer is DEVICE memory on the
 *    context's GPU, every `h_*` pointer is host memory; `stream` is a
 *    hipStream_t passed as void* (NULL = the default stream);
 *  - all entry points are asynchronous on `stream` unless stated otherwise and
 *    allocate nothing (graph-capturable) — scratch lives in the wf_ctx;
 *  - complex128 arrays are interleaved (re, im) doubles, as numpy stores them;
 *  - return value: 0 on success, a negative wf_status otherwise;
 *    wf_last_error_string() describes the last failure on the calling thread.
 *    The Python layer maps WF_ERR_VALUE -> ValueError, WF_ERR_KEY -> KeyError
 *    (the exceptions the reference raises), anything else -> RuntimeError.
 */
#ifndef WFHIP_H
#define WFHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    WF_OK = 0,
    WF_ERR_VALUE = -1,   /* bad argument (reference raises ValueError)          */
    WF_ERR_KEY = -2,     /* undefined table entry (reference raises KeyError)   */
    WF_ERR_HIP = -3,     /* a HIP runtime call failed                           */
    WF_ERR_DEVICE = -4,  /* a kernel reported a fault (e.g. scan hand-off timeout) */
    WF_ERR_NOMEM = -5
} wf_status;

typedef struct wf_ctx wf_ctx;

/* ---- library / context --------------------------------------------------- */
const char *wf_version(void);
const char *wf_last_error_string(void);

/* One context per GPU: owns the scan descriptors, LFSR jump tables and the
 * device fault word.  Synchronous (allocates).  `max_samples` sizes the scan
 * scratch (it grows on demand outside graph capture). */
int wf_ctx_create(int device, wf_ctx **out);
int wf_ctx_destroy(wf_ctx *ctx);
/* Retire a context without freeing it: stops the persistent per-symbol server (SOQPSKTrellisDetector.iteration,
 * waveforms/viterbi/algorithm.py:57-101, is served by one), drains the side stream of pipelined links and refuses to
 * start a new server afterwards.  The handle stays valid for wf_link_join / wf_viterbi4_iteration_quiesce /
 * wf_ctx_destroy — what the reference's objects do from finalisers after interpreter exit began
 * (examples/soqpsk_detection.py keeps its detector at module level).  Idempotent, synchronous. */
int wf_ctx_retire(wf_ctx *ctx);
/* Synchronises `stream`, returns WF_ERR_DEVICE if any kernel since the last
 * check raised the fault word (and clears it). */
int wf_ctx_check(wf_ctx *ctx, void *stream);
/* Per-context options: everything that tunes or instruments the library is a field of the context set through
 * this call — the library reads no environment variable and keeps no process-wide switch (the reference's objects
 * carry their own configuration the same way: SOQPSKTrellisDetector(length, differantial_encoding),
 * waveforms/viterbi/algorithm.py:19-42).  Values are int64; 0 is every option's default but WF_OPT_PIPE_RESERVE_CUS's.  Unknown key or a value
 * outside the option's range: WF_ERR_VALUE.  Takes effect for calls issued afterwards on this context. */
typedef enum {
    WF_OPT_CPM_FORM = 0,          /* generic CPM detector: 0 choose by estimated time, 1 row form, 2 lane form (where compiled in) */
    WF_OPT_CPM_CHUNK_CALLS = 1,   /* calls per chunk of the generic CPM detector (any form); 0 = the library's choice */
    WF_OPT_DET_REPAIR = 2,        /* chunk-parallel detectors: 0 repair chunks whose proof failed (cascading: see
                                   * wf_viterbi_repaired), 1 only COUNT them (wf_viterbi4_unmerged) — tests of the proof */
    WF_OPT_DET_FINAL_VERIFY = 3,  /* 1: after the repairs compare every chunk boundary once more and count what still
                                   * differs in wf_viterbi4_unmerged (an internal-consistency check; always 0) */
    WF_OPT_ITERATION_SERVER = 4,  /* wf_viterbi4_iteration_host: 0 persistent server, 1 one launch + synchronise per call */
    WF_OPT_MCB_TAIL_PERMILLE = 5, /* one-kernel front end: resident-slot-fulls of tail tiles x 1000; 0 = default, -1 = none */
    WF_OPT_PIPE_RESERVE_CUS = 6,  /* pipelined SOQPSK link (wf_link_config.fuse bit 5): the order of a block's kernels.  A context starts with -1.
                                   * N >= 1: each block's prologue (PRBS + precoder, carry kernels) beside the previous block's front end
                                   * (on the caller's stream; on a stream of the library's for a caller on the NULL stream), the front-end
                                   * kernel on a stream whose CU mask leaves N compute units free, launched behind the previous block's
                                   * detector; -1: the same without a mask for the forms it was measured faster for — the short
                                   * (pulse-truncation) bank: 0.435 against 0.459 ms per block at 8 samples per symbol, 0.564 against 0.591
                                   * at 10 — and the order of 0 for the long (PAM) bank (0.72 against 0.654 ms: profiles/order_ab_headline.log,
                                   * order_ab_others.log); 0: front end and prologue on the caller's stream, the prologue between two
                                   * front ends.  Set before the context's first pipelined block. */
    WF_OPT_CPM_SAMPLES_MIN_CALLS = 7, /* wf_cpm_viterbi_detect_samples / wf_cpm_link_config.fuse bit 7, 16-state lane form: shortest burst (calls) that
                                   * takes the samples form; 0 = the library's 6e6 (below it rows + the row form are faster: one lane per chunk leaves
                                   * most of a short burst's chunks to warm-up), otherwise >= 4096 — tests run the form on bursts an oracle can follow */
    WF_OPT_SOFT_CHUNK_CALLS = 8,  /* wf_viterbi4_soft: rows per chunk (1 .. 8192); 0 = the library's choice (wf_viterbi4_soft_geometry) */
    WF_OPT_CPM_SOFT_CHUNK_CALLS = 9, /* wf_cpm_soft: calls per chunk (1 .. 8192); 0 = the library's choice (wf_cpm_soft_geometry) */
    WF_OPT_COUNT = 10
} wf_option;
int wf_ctx_set_option(wf_ctx *ctx, int key, int64_t value);
int wf_ctx_get_option(wf_ctx *ctx, int key, int64_t *value);
/* Two link options are promises about small device tables (wf_link_config.d_mf_factor; wf_cpm_link_config.fuse bit 6): the
 * library checks each on a host copy the first time it sees the table's ADDRESS on a context and remembers the verdict.  Whoever
 * frees or rewrites such a table calls this before the address can mean something else (the Python links do so when they are
 * created): every promise is then checked again on its next use.  (Reference: its objects own their tables,
 * examples/soqpsk_detection.py:134-173 builds them per run — nothing to invalidate there.) */
int wf_ctx_forget_promises(wf_ctx *ctx);

/* ---- K1: PRBS ------------------------------------------------------------
 * GLFSR.next_bit x n   (waveforms/glfsr/glfsr.py:6-19, pn.py:98-107).
 * Writes bits `skip .. skip+n-1` of the sequence started from `state` as one
 * u8 (0/1) per bit.  Leap-ahead by GF(2) matrix powers, bit-exact.
 * If h_state_out != NULL it receives the register after skip+n steps (host
 * arithmetic, available immediately).  `degree` in 2..64, mask as
 * generate_mask (pn.py:75-90) builds it. */
int wf_lfsr_generate(wf_ctx *ctx, int degree, uint64_t mask, uint64_t state, uint64_t skip,
                     uint8_t *d_bits, int64_t n, uint64_t *h_state_out, void *stream);

/* ---- K2: bits -> symbols ---------------------------------------------------
 * TrellisEncoder.encode (waveforms/cpm/trellis/encoder.py:17-48) for any
 * trellis of <= 16 states, <= 4 input bits per symbol.  Tables are HOST arrays,
 * dense [column][state][input]: h_next (u8) / h_out (i8), i.e. forward_map
 * (waveforms/cpm/trellis/model.py:127-137).  `i0`/`state0` are TrellisEncoder.i
 * / .state on entry; *h_state_out receives .state after the call (this one
 * value is copied back synchronously).  nbits % card != 0 -> WF_ERR_VALUE
 * (encoder.py:28-30). */
int wf_fsm_encode(wf_ctx *ctx, const uint8_t *h_next, const int8_t *h_out, int columns, int states,
                  int card, const uint8_t *d_bits, int64_t nbits, int64_t i0, int state0,
                  int8_t *d_symbols, int *h_state_out, void *stream);

/* Stateless-per-element mappers (a2'):
 *  kind 0: SOQPSKPrecoder.__call__  (waveforms/cpm/soqpsk/precoder.py:10-24),
 *          parity = precoder .i, mem0/mem1 = precoder .mem, out in {-1,0,1};
 *  kind 1: MultiHSymbolMapper.__call__ (waveforms/cpm/multih/precoder.py:9-23),
 *          parity = mapper .i AFTER its update, n must be even, out n/2 symbols;
 *  kind 2: PCMFMSymbolMapper.__call__ (waveforms/cpm/pcmfm/precoder.py:6-15). */
int wf_symbol_map(wf_ctx *ctx, int kind, const uint8_t *d_bits, int64_t n, int parity, int mem0,
                  int mem1, int8_t *d_symbols, void *stream);

/* ---- K3: zero-stuffed upsample + frequency-pulse FIR -----------------------
 * interpolated[sps:-1:sps] = symbols*h ; np.convolve(.., pulse, "same")
 * (waveforms/cpm/modulate.py:91-99).  Symbol m uses h[m % nh].  Output length
 * is wf_fir_out_len(nsym, sps, ntaps) = max((nsym+1)*sps, ntaps) — numpy's
 * "same" returns the longer operand's length. */
int64_t wf_fir_out_len(int64_t nsym, int sps, int ntaps);
int wf_upsample_fir_f64(wf_ctx *ctx, const int8_t *d_symbols, int64_t nsym, const double *d_h,
                        int nh, const double *d_pulse, int ntaps, int sps, double *d_out,
                        void *stream);

/* ---- K4: phase accumulate (mod sps) + complex exponential ------------------
 * frequency_modulate (waveforms/cpm/modulate.py:28-54):
 *   revs_k = (revs_{k-1} + f_k) mod sps ; out_k = exp(j (revs_k 2pi/sps + phi0)).
 * Single-pass chained prefix scan; `revs_in` continues a previous chunk
 * (0 for a fresh call), *d_revs_out (may be NULL) receives the final revs. */
int wf_phase_cexp_f64(wf_ctx *ctx, const double *d_freq, int64_t n, int sps, double phi0,
                      double revs_in, double *d_out_ri, double *d_revs_out, void *stream);
/* Fused K3 + K4: cpm_modulate (waveforms/cpm/modulate.py:57-101) straight from symbols
 * to the complex baseband signal, one pass over HBM (1 B in, 16*sps B out per symbol);
 * tile carries come from a symbol-rate prefix sum instead of an inter-workgroup scan.
 * Same results as wf_upsample_fir_f64 followed by wf_phase_cexp_f64 (to rounding).
 * Returns 1 — not an error — when the configuration is outside the fused kernel's
 * envelope (signal shorter than the pulse, pulse longer than 33 symbols or than a tile, more than 8
 * modulation indices — modulate.py:91-92 cycles any number: symbol i takes d_h[i mod nh]);
 * the caller then runs the two stage kernels. */
int wf_cpm_modulate_c128(wf_ctx *ctx, const int8_t *d_symbols, int64_t nsym, const double *d_h, int nh,
                         const double *d_pulse, int ntaps, int sps, double phi0, double *d_out_ri,
                         void *stream);
/* phase_modulate (waveforms/cpm/modulate.py:12-25): out = exp(j * sens * phase). */
int wf_phase_modulate_f64(wf_ctx *ctx, const double *d_phase, int64_t n, double sens,
                          double *d_out_ri, void *stream);

/* ---- K5: AWGN ---------------------------------------------------------------
 * Device counterpart of generate_complex_awgn (waveforms/noise.py:8-32) and of
 * `signal * exp(-j pi/4) + noise` (examples/soqpsk_detection.py:85-89):
 *   out_k = in_k * (rot_re + j rot_im) + sigma * (n_re + j n_im)_k
 * with (n_re, n_im)_k = Box-Muller (two 32-bit uniforms) of half a Philox4x32-10 block:
 * absolute index a = first_index + k, counter = (a >> 1, stream_id), key = seed, words
 * (x0,x1) for even a, (x2,x3) for odd a.  d_in may be NULL (pure noise).  In-place allowed. */
int wf_awgn_c128(wf_ctx *ctx, const double *d_in_ri, int64_t n, double rot_re, double rot_im,
                 double sigma, uint64_t seed, uint64_t stream_id, uint64_t first_index,
                 double *d_out_ri, void *stream);

/* The Box-Muller half of the source on caller-supplied words: sample k from
 * (d_words[2k], d_words[2k+1]) = (radius word xa, angle word xb) exactly as wf_awgn_c128
 * uses the halves of a Philox block.  |sample| <= sigma * sqrt(64 ln 2) = 6.66 sigma. */
int wf_box_muller32_c128(wf_ctx *ctx, const uint32_t *d_words, int64_t n, double sigma, double *d_out_ri,
                         void *stream);

/* ---- K6/K7: matched-filter bank ----------------------------------------------
 * nfilt complex FIRs, each np.convolve(r, taps[f], "same") sampled at
 * n = first + k*step, k < ncols   (examples/soqpsk_detection.py:141-156 PT bank,
 * :164-173 PAM bank with the pseudo-symbol weights folded into the taps,
 * :189-196 decimation).  d_taps is nfilt x ntaps complex128; output is
 * ncols x nfilt complex128 (one row per detector call).  step = 1, first = 0,
 * ncols = nsamp gives the full-rate bank.  Requires nsamp >= ntaps. */
int wf_mf_bank_c128(wf_ctx *ctx, const double *d_r_ri, int64_t nsamp, const double *d_taps_ri,
                    int nfilt, int ntaps, int64_t first, int step, int64_t ncols,
                    double *d_out_ri, void *stream);

/* Fused K5 + K6: the channel of wf_awgn_c128 applied while the matched-filter bank stages
 * its input (received samples never materialise in HBM).  Output identical to
 * wf_awgn_c128 followed by wf_mf_bank_c128 with the same noise coordinates. */
int wf_awgn_mf_bank_c128(wf_ctx *ctx, const double *d_signal_ri, int64_t nsamp, double rot_re, double rot_im,
                         double sigma, uint64_t seed, uint64_t stream_id, uint64_t first_index,
                         const double *d_taps_ri, int nfilt, int ntaps, int64_t first, int step,
                         int64_t ncols, double *d_out_ri, void *stream);

/* ---- K8-K10: SOQPSK 4-state Viterbi detector ---------------------------------
 * SOQPSKTrellisDetector (waveforms/viterbi/algorithm.py:18-101) with
 * length = 2: for every row of d_mf (ncalls x 3 complex128, alpha = -2,0,+2)
 * element [0] of the bits / symbols arrays that .iteration() returns.
 * Chunk-parallel: each thread re-derives the path metrics over `warmup` rows
 * before its chunk; decisions equal the sequential detector's once survivors
 * have merged (warmup >= 32 recommended, 0 = library default).
 * d_state (may be NULL) is the detector state carried across calls for streaming:
 * [i, M0[4], inc_prev[8], pad[3]] + 16 doubles of staging (32 doubles,
 * zero-initialised = a fresh detector); NULL = a fresh detector, no carry-out. */
int wf_viterbi4_detect(wf_ctx *ctx, const double *d_mf_ri, int64_t ncalls, int differential,
                       int warmup, uint8_t *d_bits, int8_t *d_syms, double *d_state,
                       void *stream);
/* The same for ANY window `length` in 1 .. 64 (waveforms/viterbi/algorithm.py:19-42: `length` is a free
 * parameter; window loop :69-87, depth-`length` traceback :90-98).  Odd lengths included, literally: there the
 * reference pairs a row's increments (:57-63, section i % 2) with the branches of the other section (:69-87), and
 * at length 1 the stage updates its metrics column in place.  For every row, element [0] of what .iteration()
 * returns — the stage-0 branch of the path that ends in the first arg-min state after `length` - 1 stages of look-ahead.  Chunk-parallel with the
 * same on-device proof (wf_viterbi4_unmerged).  d_state (may be NULL): wf_viterbi4_window_state_bytes() bytes,
 * zero-initialised = a fresh detector, carried across calls of the same length. */
int wf_viterbi4_detect_window(wf_ctx *ctx, const double *d_mf_ri, int64_t ncalls, int length, int differential,
                              int warmup, uint8_t *d_bits, int8_t *d_syms, double *d_state, void *stream);
int64_t wf_viterbi4_window_state_bytes(void);
/* The batch detectors are chunk-parallel: every chunk re-derives the path metrics over `warmup` rows before
 * its own calls.  Each launch then PROVES on the device that the state a chunk started from is bitwise the state
 * the previous chunk ended with — the condition under which all decisions are those of the sequential
 * SOQPSKTrellisDetector (waveforms/viterbi/algorithm.py:44-101) — and REPAIRS what fails: the chunk's own calls
 * run again from the true state; a chunk whose end state changed hands it to the next chunk, which is run again in
 * turn, round after round until no boundary differs (worst case: the sequential detector).  So the result never
 * depends on `warmup`; the warm-up only sets how often the repair runs.
 * wf_viterbi4_unmerged: chunks left unproven since the last reset (synchronises `stream`).  With the default
 * options this is always 0; it counts only under WF_OPT_DET_REPAIR = 1 (repairs off) or when
 * WF_OPT_DET_FINAL_VERIFY finds an inconsistency. */
int wf_viterbi4_unmerged(wf_ctx *ctx, int64_t *h_count, int reset, void *stream);
/* *h_count = chunk repairs run since the last reset, every round counted (synchronises `stream`).
 * wf_viterbi_cascaded: of those, the repairs whose chunk ended in a different state than before and therefore
 * handed on to the next chunk.  (Build-defined like the proof itself: the reference's detector is one sequential
 * loop, algorithm.py:44-101.) */
int wf_viterbi_repaired(wf_ctx *ctx, int64_t *h_count, int reset, void *stream);
int wf_viterbi_cascaded(wf_ctx *ctx, int64_t *h_count, int reset, void *stream);

/* ---- SOQPSK 4-state soft output: max-log-MAP, per-bit LLRs ------------------------------------------------------------
 * A burst of `ncalls` rows (free start, free end) over the trellis, the branch increments and the column schedule of
 * SOQPSKTrellisDetector (waveforms/viterbi/algorithm.py:44-101: inc_k(b) = Re(state_exp_term[start b] * z_k[idx(out b)]),
 * row k is section k with column k % 2, metrics minimised).  In float64 and in exactly this order of operations:
 *   ã_0 = 0;   a'_{k+1}(s') = min_{b: end b = s'} (ã_k(start b) + inc_k(b));      ã_{k+1} = a'_{k+1} - min_s a'_{k+1}(s)
 *   b̃_N = 0;   b'_k(s)      = min_{b: start b = s} (inc_k(b) + b̃_{k+1}(end b));   b̃_k     = b'_k - min_s b'_k(s)
 *   d_llr[k] = λ_k = min_{b: inp b = 1} ((ã_k(start b) + inc_k(b)) + b̃_{k+1}(end b)) - min_{b: inp b = 0} (the same)
 *   d_bits[k] = λ_k < 0  (λ > 0 favours bit 0).
 * λ is in metric units, no scale baked in.  Alignment: transmitted bit j pairs with λ_{j+1} (the length-2 hard detector's
 * output k + 1 is its decision on section k).  The hard decisions are the maximum-likelihood sequence under the
 * reference's metric: they equal the long-window detector's (wf_viterbi4_detect_window, length >= 8), NOT the length-2
 * detector's, and need not have fewer bit errors than it.
 * d_rows: 48-byte rows (3 complex128, alpha = -2, 0, +2; 16-byte aligned) or, row_bytes = 32, the links' detector-packed
 * rows {Re z1, Im z1, a, b} (wf_link_config.fuse bit 2).  Each call is a fresh burst.  Chunk-parallel with the proof and
 * cascading repair of the hard detectors in BOTH directions (forward metrics at every chunk start, backward metrics at
 * every chunk end), so the result is bitwise the definition whatever `warmup` (rows, 0 = library default) and
 * WF_OPT_SOFT_CHUNK_CALLS are; WF_OPT_DET_REPAIR / WF_OPT_DET_FINAL_VERIFY act as for the hard detectors, and the
 * repairs and unproven chunks (forward and backward) are counted in wf_viterbi_repaired / wf_viterbi4_unmerged.
 * Scratch: the context's detector scratch (wf_viterbi4_soft_geometry [3] bytes).  row_bytes not 32 / 48, ncalls < 1,
 * warmup < 0 or a NULL pointer: WF_ERR_VALUE before the context is touched.  (The generic CPM detectors' soft output,
 * ARTM and PCM/FM: wf_cpm_soft, behind wf_cpm_count_errors below.) */
int wf_viterbi4_soft(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int row_bytes, int differential, int warmup,
                     double *d_llr, uint8_t *d_bits, void *stream);
/* What wf_viterbi4_soft launches for this burst on this context: h_geom[0] rows per chunk, [1] chunks (= lanes),
 * [2] warm-up rows actually used, [3] scratch bytes. */
int wf_viterbi4_soft_geometry(wf_ctx *ctx, int64_t ncalls, int warmup, int64_t *h_geom);

/* wf_viterbi4_soft with a per-row prior on the input bit and EXTRINSIC output: the inner detector of iterative detection
 * and decoding.  Everything of wf_viterbi4_soft holds (rows, alignment, warm-up, chunking, options, counters, scratch:
 * wf_viterbi4_soft_geometry describes this call too) with, in float64 and in exactly this order of operations:
 *   π_k = apriori_scale * (double)d_apriori[k]                               (0 when d_apriori is NULL)
 *   inc'_k(b) = inc_k(b) + π_k when inp b = 1, inc_k(b) otherwise            (one float64 addition)
 *   ã, b̃: the recursions of wf_viterbi4_soft with inc' in place of inc
 *   d_ext[k]  = λᵉ_k = min_{b: inp b = 1} ((ã_k(start b) + inc_k(b)) + b̃_{k+1}(end b)) - min_{b: inp b = 0} (the same)
 *               (the CHANNEL-only inc_k in section k: the prior of bit k is never added, so none is subtracted)
 *   d_bits[k] = (λᵉ_k + π_k) < 0
 * π > 0 favours bit 0, as λ does.  d_apriori: ncalls float32 (4-byte aligned), finite; row k's prior is d_apriori[k], so the
 * prior of transmitted bit j goes to d_apriori[j + 1].  With d_apriori NULL the result is bitwise wf_viterbi4_soft's.
 * A prior may be negative, so an increment inc' may be negative or -0; the implementation relies on this instead of on
 * non-negative increments: a normalised metric ã, b̃ is x - min x, which is >= +0 and never -0, a sum with an operand that
 * is not -0 is not -0, so no operand of a min is ever -0, equal operands are bitwise equal and the min does not depend
 * on the order in which a machine takes it.  Rows and priors must be finite.  apriori_scale not finite, or any
 * argument wf_viterbi4_soft refuses: WF_ERR_VALUE before the context is touched. */
int wf_viterbi4_soft_apriori(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int row_bytes, int differential, int warmup,
                             const float *d_apriori, double apriori_scale, double *d_ext, uint8_t *d_bits, void *stream);

/* ---- Live windows: the detector pass of an iterative loop on the open codewords only -----------------------------------------
 * (The reference has no coding layer; these entry points are defined here.)
 * wf_idd_windows: which rows of a burst a detector pass still has to work on, from the decoder's freeze states, ON THE
 * DEVICE (the loop never synchronises with the host).  d_state: ncw bytes, 0 = open, as wf_ldpc_decode_ext leaves them.
 * Codeword b occupies the rows [a_b, e_b) of the nrows detector rows, a_b = first + b P, e_b = a_b + n_tx, with
 * first = row_offset + p̂ + L and p̂ = the first int64 of the 32-byte lock record of wf_frame_search READ FROM DEVICE MEMORY
 * (d_lock NULL: p̂ = 0).  Codewords sent back to back behind wf_viterbi4_soft: row_offset = 1, d_lock = NULL, L = 0, P = n_tx
 * (coded bit j is row j + 1); framed: row_offset = 1, the lock, the marker length L, P = L + n_tx.  With the guard G >= 0 rows:
 *   windows = []
 *   for b = 0 .. ncw - 1 with d_state[b] == 0:
 *       s = max(0, a_b - G) & ~1          (even: row k is trellis column k % 2, a window keeps the burst's parity)
 *       e = min(nrows, e_b + G)
 *       if e <= s: continue               (the span lies outside the burst: a wrong lock)
 *       if windows and s - windows[-1].e < G:  windows[-1].e = max(windows[-1].e, e)        (merge)
 *       else:                                  windows.append((s, e))
 * d_table (int64, 4 + 2 ncw words, 8-byte aligned) receives [0] W = the number of windows, [1] the live rows sum (e - s),
 * [2] the codewords with state 0, [3] 0, then the W pairs (s, e) in increasing order; the words behind the pairs are not
 * specified.  Asynchronous on `stream`; nothing is returned to the host.  waveforms_amd/encoding/live.py states the same in
 * numpy.  A NULL ctx / d_state / d_table, ncw < 1 or > 2^31, nrows < 1, n_tx < 1, P < n_tx, a negative row_offset, L or G, a
 * pointer not 8-byte aligned: WF_ERR_VALUE before the context is touched. */
int wf_idd_windows(wf_ctx *ctx, const uint8_t *d_state, int64_t ncw, int64_t nrows, int32_t n_tx, int64_t P, int64_t row_offset,
                   const void *d_lock, int32_t L, int64_t G, int64_t *d_table, void *stream);
/* wf_viterbi4_soft_apriori over the windows of such a table (d_windows, read on the device; any table of this form will do:
 * W <= max_windows windows with even starts, 0 <= s < e <= ncalls, in increasing order and disjoint).  For every window (s, e),
 * d_ext[s .. e) and d_bits[s .. e) are BITWISE what wf_viterbi4_soft_apriori returns for the burst d_rows + s rows,
 * ncalls = e - s, d_apriori + s: free start at s, free end at e, the same definition, the same independence of `warmup` and
 * WF_OPT_SOFT_CHUNK_CALLS (the proof and the cascading repair run per window: a window's first chunk starts from zero
 * metrics at s, its last one from zero at e, exact as the ends of a burst are), the same options and counters.  Rows outside
 * every window are NOT WRITTEN; W = 0 writes nothing and runs no chunk.  d_rows, d_apriori, d_ext and d_bits are the whole
 * burst's (ncalls rows); d_apriori must not be NULL (the first pass of a block, where no codeword is frozen, is the plain
 * detector's).  W and the live rows are known on the device only: the launches are sized for every row live plus one
 * partial chunk per window (max_windows of them: ncw for a table of wf_idd_windows) and so is the context's detector
 * scratch; a lane without a live chunk leaves at once.  A table that is not of the form above raises the context's fault
 * word (wf_ctx_check: WF_ERR_DEVICE) and no row is touched.  A NULL pointer, max_windows < 1, a table not 8-byte aligned or
 * any argument wf_viterbi4_soft_apriori refuses: WF_ERR_VALUE before the context is touched. */
int wf_viterbi4_soft_apriori_windows(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int row_bytes, int differential, int warmup,
                                     const float *d_apriori, double apriori_scale, const int64_t *d_windows, int64_t max_windows,
                                     double *d_ext, uint8_t *d_bits, void *stream);

/* wf_viterbi4_detect + wf_count_errors in one call (fresh detector): decision k is
 * compared with reference element k - skip for 0 <= k - skip < ncompare
 * (examples/soqpsk_detection.py:201-209: skip = length); counts are ADDED to d_counts[0..1]. */
int wf_viterbi4_detect_count(wf_ctx *ctx, const double *d_mf_ri, int64_t ncalls, int differential, int warmup,
                             uint8_t *d_bits, int8_t *d_syms, const uint8_t *d_ref_bits,
                             const int8_t *d_ref_syms, int skip, int64_t ncompare, int64_t *d_counts,
                             void *stream);
/* One literal .iteration() for any window `length` <= 64 (algorithm.py:44-101),
 * detector state resident on the device (wf_viterbi4_state_bytes(length) bytes,
 * zero-initialised = a new detector).  d_mf3: 3 complex128.  Outputs: `length`
 * doubles each, as the reference returns. */
int64_t wf_viterbi4_state_bytes(int length);
int wf_viterbi4_iteration(wf_ctx *ctx, void *d_state, int length, int differential,
                          const double *d_mf3_ri, double *d_bits_out, double *d_syms_out,
                          void *stream);

/* The same call with HOST operands (h_mf3: 3 complex128; outputs `length` doubles each), for the
 * reference's per-symbol loop (examples/soqpsk_detection.py:189-198): one launch + one stream
 * synchronise through pinned, device-mapped staging owned by the context.  Synchronous.
 * `d_state` must be initialised (its zero fill complete, not merely enqueued) before the first call
 * made for it: the call only synchronises `stream` when `d_state` differs from the previous call's. */
int wf_viterbi4_iteration_host(wf_ctx *ctx, void *d_state, int length, int differential,
                               const double *h_mf3_ri, double *h_bits_out, double *h_syms_out, void *stream);
/* Diagnostic: device-side timing of the last request wf_viterbi4_iteration_host's persistent server answered, in
 * microseconds: {request read from host memory, cache check, the iteration itself, write-through + answer}. */
int wf_viterbi4_iteration_server_timing(wf_ctx *ctx, double *h_us4);
/* wf_viterbi4_iteration_host answers BEFORE the detector state has been written back to device memory (about a
 * microsecond later).  Call this before anything else reads, overwrites or frees a `d_state` that was passed to
 * it (the next wf_viterbi4_iteration_host call needs nothing: one server, in order).  No-op without a server.
 * (Reference: the state is the detector object's own arrays, waveforms/viterbi/algorithm.py:36-42.) */
int wf_viterbi4_iteration_quiesce(wf_ctx *ctx);
/* The detector's public state arrays as the reference keeps them on every instance (waveforms/viterbi/algorithm.py:25-42:
 * bi_history float64[8][length], metrics float64[4][length], path uint8[4][length]; :44 the call counter `i`), read from a
 * device-resident state of wf_viterbi4_iteration / _host into host arrays of those shapes (row-major).  Quiesces the per-symbol
 * server first; synchronous.  h_calls may be NULL. */
int wf_viterbi4_state_read(wf_ctx *ctx, const void *d_state, int length, int64_t *h_calls, double *h_bi_history,
                           double *h_metrics, uint8_t *h_path, void *stream);

/* ---- K11: error counting ------------------------------------------------------
 * examples/soqpsk_detection.py:200-209: number of j < m with
 * det_syms[j] != ref_syms[j] and with det_bits[j] != ref_bits[j]; the two counts
 * are ADDED to d_counts[0], d_counts[1] (int64; zero them first). */
int wf_count_errors(wf_ctx *ctx, const int8_t *d_det_syms, const int8_t *d_ref_syms,
                    const uint8_t *d_det_bits, const uint8_t *d_ref_bits, int64_t m,
                    int64_t *d_counts, void *stream);

/* ---- a5 helper: normalized time axis -----------------------------------------
 * np.linspace(0, N+1, (N+1)*sps, endpoint=False) (waveforms/cpm/modulate.py:81-88):
 * out[k] = k * step. */
int wf_time_axis_f64(wf_ctx *ctx, int64_t n, double step, double *d_out, void *stream);

/* ---- device-resident link (one Monte-Carlo trial block / one bench step) -------
 * PRBS -> TrellisEncoder(SOQPSKTrellis4x2[DiffEncoded]) -> cpm_modulate -> *exp(-j pi/4)
 * + AWGN -> matched-filter bank sampled at (n + timing_offset) % sps == 0 ->
 * SOQPSKTrellisDetector(length = 2) -> error count: the per-waveform body of
 * examples/soqpsk_detection.py:45-216, every stage one of the kernels above, all
 * intermediates in the caller's HBM workspace.  d_counts[0] += symbol errors,
 * d_counts[1] += bit errors; *h_compared (host, may be NULL) = number of symbols
 * compared (min_size of :204). */
typedef struct {
    int64_t nsym;           /* symbols (= bits) in the block                          */
    int sps;
    int degree;             /* PRBS register: degree, mask, start state, bits to skip */
    uint64_t mask, state, skip;
    int differential;       /* 1: SOQPSKTrellis4x2DiffEncoded, 0: SOQPSKTrellis4x2     */
    const double *d_h;      /* device: modulation index (1 double)                    */
    const double *d_pulse;  /* device: frequency pulse, ntaps doubles                 */
    int ntaps;
    const double *d_mf_taps; /* device: mf_nfilt x mf_ntaps complex128                */
    int mf_ntaps, mf_nfilt; /* mf_nfilt must be 3                                     */
    int timing_offset;      /* -1 for the PT bank, 0 for PAM-TG (:184-187)            */
    double sigma;           /* noise std-dev per real dimension                       */
    uint64_t seed, stream_id; /* Philox key / subsequence                             */
    int warmup;             /* Viterbi chunk warm-up, 0 = default                     */
    int fuse;               /* bit 0: fused modulator (wf_cpm_modulate_c128) instead   */
                            /* of the FIR + phase-scan stage kernels; bit 1: AWGN      */
                            /* inside the MF bank (wf_awgn_mf_bank_c128); bit 2 (with  */
                            /* bit 1, 3-filter bank, sps 8): the bank writes only the  */
                            /* 4 real components per call the 4-state detector reads   */
                            /* ({Re z1, Im z1, Re|Im z0, Im|Re z2}: 32 B rows, not 48);  */
                            /* bit 3 (with bits 0-2, 9-tap bank): modulator, channel and */
                            /* bank in ONE kernel — the baseband samples never reach HBM */
                            /* (rows bit-identical to bits 0-2; falls back to them when  */
                            /* the pulse is outside the kernel: > 9 symbols, sps != 8);  */
                            /* bit 4 (16): PRBS and precoder through the generic kernels */
                            /* (wf_lfsr_generate + the three-kernel wf_fsm_encode scan)   */
                            /* instead of the link's one-launch form (same bits and      */
                            /* symbols; bursts over 3.3e7 symbols take the generic form); */
                            /* bit 5 (32, with the one-kernel front end): the detector   */
                            /* and the error count of a block run on the context's side  */
                            /* stream and overlap the front end of the NEXT wf_link_run  */
                            /* on the same context; the workspace then holds two sets of */
                            /* intermediates (wf_link_workspace_bytes says so), used     */
                            /* alternately; counts complete after wf_link_join /         */
                            /* wf_ctx_check on the stream that reads them                 */
    int event_slot;         /* -1: off; 0..WF_LINK_EVENT_SLOTS-1: record HIP events    */
                            /* around every stage into that slot (wf_link_stage_ms)   */
    const double *d_mf_factor; /* device, optional (NULL: none): a long bank (the PAM    */
                            /* detector's, mf_ntaps != sps + 1) FACTORED as the reference */
                            /* computes it (examples/soqpsk_detection.py:158-173): two    */
                            /* real filters b_0, b_1 (mf_ntaps doubles each) and the 3 x 2 */
                            /* complex combination G (12 doubles, G[s][k] as re, im), with */
                            /* d_mf_taps[s] == sum_k G[s][k] b_k.  The one-kernel front end */
                            /* then runs two real filters instead of three complex ones    */
                            /* (a third fewer matrix instructions); every other path reads */
                            /* d_mf_taps.  The identity is CHECKED (host copy, 1e-12 of the */
                            /* largest tap) the first time these pointers are seen on a     */
                            /* context: a factorisation that does not reproduce the taps is */
                            /* WF_ERR_VALUE.  Do not rewrite the tables in place afterwards. */
} wf_link_config;
#define WF_LINK_EVENT_SLOTS 64
#define WF_LINK_STAGES 8    /* prbs, encode, fir, phase, awgn, mfbank, viterbi, count */
int64_t wf_link_workspace_bytes(const wf_link_config *cfg);
int wf_link_run(wf_ctx *ctx, const wf_link_config *cfg, void *d_workspace, int64_t workspace_bytes,
                int64_t *d_counts, int64_t *h_compared, void *stream);
/* Elapsed milliseconds of the WF_LINK_STAGES stages of the run that last used
 * `event_slot` (HIP events on the run's own stream).  Synchronises on that slot's
 * final event. */
int wf_link_stage_ms(wf_ctx *ctx, int event_slot, float *h_ms);

/* `stream` waits for the detectors and error counters that wf_link_run calls with fuse bit 5 left on the context's
 * side stream: call it (or wf_ctx_check, which includes it) on the stream that will read or reset the counters, or
 * reuse the workspace for something else.  No-op for a context that never ran a pipelined block.
 * (Reference: the loop body of examples/soqpsk_detection.py:45-216 is sequential; this is a scheduling call.) */
int wf_link_join(wf_ctx *ctx, void *stream);

/* Workspace offsets of a wf_link_run block, for callers that want the intermediates:
 * info8 = {ncols, one_kernel, off(detected bits), off(detected symbols), off(signal), row_bytes,
 *          signal samples, off(MF rows)} (offsets in bytes into the workspace).  one_kernel = 1: fuse = 15 runs
 *          modulator + channel + bank as ONE kernel for this configuration (3 x (sps + 1) bank at 8, 10 or 20
 *          samples per symbol, pulse of at most 9 symbols); row_bytes = 32 when the MF rows area holds the 4
 *          doubles per call the detector reads (fuse bit 2 in effect), else 16 * mf_nfilt. */
int wf_link_layout(const wf_link_config *cfg, int64_t *info8);

/* ---- streaming link (continuous stream in chunks) -------------------------------
 * The same chain over a stream of cfg->nsym symbols, `chunk_symbols` detector calls per
 * call, chunk_index = 0, 1, ... in order on one stream.  Neighbouring context is
 * re-generated as a halo (PRBS leap-ahead, counter-based noise, one modulator tile of
 * samples) or carried in `d_state` (WF_LINK_STREAM_STATE_BYTES, zero-initialised before
 * chunk 0: Viterbi state, encoder state, modulator phase).  Decisions and error counts
 * equal wf_link_run over the whole stream.  chunk_symbols must be a multiple of the
 * modulator tile (wf_mod_tile_geometry) and of 128.  Requires the fused modulator. */
#define WF_LINK_STREAM_STATE_BYTES 512
int wf_mod_tile_geometry(int sps, int ntaps, int64_t nsym_total, int64_t *tile_len, int64_t *sym_per_tile,
                         int64_t *ntiles_total);
int64_t wf_link_stream_workspace_bytes(const wf_link_config *cfg, int64_t chunk_symbols);
/* info8 = {calls in the chunk, first call index, off(detected bits), off(detected symbols),
 *          off(signal), global index of signal[0], signal samples resident, off(MF rows)} */
int wf_link_stream_layout(const wf_link_config *cfg, int64_t chunk_symbols, int64_t chunk_index, int64_t *info8);
int wf_link_stream_chunk(wf_ctx *ctx, const wf_link_config *cfg, int64_t chunk_symbols, int64_t chunk_index,
                         void *d_state, void *d_workspace, int64_t workspace_bytes, int64_t *d_counts,
                         int64_t *h_compared, void *stream);
/* Parts of a chunk, for callers that pipeline chunks on two streams with a workspace AND a wf_ctx
 * each (the parts of one chunk use the same pair).  `phases` is a bit set; each part needs the same
 * part of the previous chunk (its carry in d_state) and the earlier parts of its own chunk:
 *   bit 0 (1): PRBS, encoder, modulator carries          (carries: encoder state, modulator phase)
 *   bit 2 (4): modulator + channel + bank                 (with fuse bit 3: no carry of its own)
 *   bit 1 (2): detector + error count                     (carry: detector state)
 * phases = 7: the whole chunk = wf_link_stream_chunk. */
int wf_link_stream_chunk_phase(wf_ctx *ctx, const wf_link_config *cfg, int64_t chunk_symbols, int64_t chunk_index,
                               void *d_state, void *d_workspace, int64_t workspace_bytes, int64_t *d_counts,
                               int64_t *h_compared, int phases, void *stream);
/* Steady state for hipGraph replay: the launch sequence of an INTERIOR chunk with the only
 * two per-chunk quantities (PRBS position, noise counter) kept in d_state and advanced on the
 * device, so every call issues identical launches.  Use: chunk 0 with wf_link_stream_chunk,
 * capture ONE wf_link_stream_steady call (hipStreamBeginCapture / torch.cuda.graph) and
 * replay it once per interior chunk 1, 2, ... (wf_link_stream_interior tells which chunks
 * qualify; d_state's position words start at zero and every call ends by advancing them one
 * chunk), then finish the remaining chunk(s) with wf_link_stream_chunk.  Allocates and
 * synchronises nothing.  Same results as wf_link_stream_chunk. */
int wf_link_stream_interior(const wf_link_config *cfg, int64_t chunk_symbols, int64_t chunk_index);
int wf_link_stream_steady(wf_ctx *ctx, const wf_link_config *cfg, int64_t chunk_symbols, void *d_state,
                          void *d_workspace, int64_t workspace_bytes, int64_t *d_counts, int64_t *h_compared,
                          void *stream);
/* wf_link_stream_steady in the parts of wf_link_stream_chunk_phase (`phases` bits 0 / 2 / 1), each advancing its
 * own position word at its end: a PIPELINE of interior chunks on two streams (workspace and wf_ctx per stream,
 * one event per part) can be captured as ONE hipGraph and replayed. */
int wf_link_stream_steady_phase(wf_ctx *ctx, const wf_link_config *cfg, int64_t chunk_symbols, void *d_state,
                                void *d_workspace, int64_t workspace_bytes, int64_t *d_counts, int64_t *h_compared,
                                int phases, void *stream);

/* ---- generic CPM trellis detector (ARTM multi-h, PCM/FM) ---------------------------
 * The reference has NO detector for these waveforms — only their modulator side
 * (waveforms/cpm/multih/pulse_filters.py:11-23, precoder.py:9-23, waveforms/cpm/pcmfm/) and the
 * state-space theory (notes/cpm/cpm.md:52-140, N_S = p M^(L-1)).  These entry points implement the
 * detector DEFINED by oracle/cpm_oracle.c (sequential, build-defined): tilted-phase states of
 * notes/cpm/cpm.md:100-140, pulse-truncation matched filters in the manner of
 * examples/soqpsk_detection.py:134-156, and the conventions of waveforms/viterbi/algorithm.py:57-98
 * (increment Re(rotation * mf) minimised, strict '<', first arg-min, min-normalised metrics, one
 * decision per call from the best state).
 *
 * State = (phase class v mod NC, the Lp-1 previous symbols); NC < p carries the phase index per
 * survivor.  At most 16 states: NC * M^(Lp-1) <= 16; M in {2, 4}; nh in {1, 2}; Lp in 1..3. */
typedef struct {
    int M;          /* alphabet size: alpha = 2 U - (M - 1), U = 0 .. M-1                      */
    int p;          /* modulation indices K[i] / p, symbol m uses K[m % nh]                    */
    int nh;
    int K[2];
    int Lp;         /* symbols per matched filter (pulse truncation length)                    */
    int NC;         /* phase classes in the trellis state (divides p)                          */
    int D;          /* decision delay: call n decides symbol n - D + 1;  D * log2(M) <= 64     */
} wf_cpm_detector_config;

/* Matched-filter rows: row n, filter f = sum_k r[start0 + n*sps + k] * conj(T[n % nh][f][k]),
 * k < ntm.  d_templates: nh x nfilt x ntm complex128 (nfilt = M^Lp, index f = u_0 + M u_1 + ...),
 * d_rows: ncalls x nfilt complex128.  Samples outside [0, nsamp) count as zero. */
int wf_cpm_mf_rows_c128(wf_ctx *ctx, const double *d_r_ri, int64_t nsamp, const double *d_templates_ri, int nh,
                        int nfilt, int ntm, int64_t start0, int sps, int64_t ncalls, double *d_rows_ri,
                        void *stream);

/* The same rows from CLEAN samples with the channel of wf_awgn_c128 applied while staging
 * (derotation by rot, Philox noise of the given seed / stream / first index): identical to
 * wf_awgn_c128 followed by wf_cpm_mf_rows_c128, without the noisy samples ever being stored. */
int wf_cpm_awgn_mf_rows_c128(wf_ctx *ctx, const double *d_signal_ri, int64_t nsamp, double rot_re, double rot_im,
                             double sigma, uint64_t seed, uint64_t stream_id, uint64_t first_index,
                             const double *d_templates_ri, int nh, int nfilt, int ntm, int64_t start0, int sps,
                             int64_t ncalls, double *d_rows_ri, void *stream);

/* The detector over ncalls rows.  d_rot_cs: 2p pairs (cos, sin)(pi r / p) (caller-computed so that
 * oracle and device rotate with the same doubles).  d_decisions[k] (uint8) = the U decided at call
 * k, i.e. of symbol n0 + k - D + 1 (n0 = calls already made on d_state; entries with
 * n0 + k < D - 1 are written as 0).  Trellises of up to 256 states (N_S = NC M^(Lp-1), notes/cpm/cpm.md:128-140: up to 16
 * in one 16-lane group, 17 .. 64 — the 64-state ARTM design — one wave per detector, 65 .. 256 — the full ARTM trellis
 * p M^(L-1) = 256 with its 64 matched filters per symbol — one workgroup per detector; pulses of 2 or 3 symbols there).
 * Chunk-parallel like wf_viterbi4_detect: each 16-lane group
 * re-derives metrics, phase indices and decision registers over `warmup` rows (0 = default) and
 * every launch verifies bitwise that a chunk started from what its predecessor ended with
 * and repairs the chunks for which that failed, cascading into the following chunks where needed
 * (wf_viterbi4_unmerged, wf_viterbi_repaired): decisions are the sequential detector's whatever the warm-up.  d_state (WF_CPM_STATE_BYTES, zeroed = fresh detector,
 * may be NULL) carries the detector across calls. */
#define WF_CPM_STATE_BYTES 16384
/* Which of its forms wf_cpm_viterbi_detect runs for this trellis, burst length and warm-up: info4[0] = 3 the quad form
 * (65 .. 256 states: thread = state, one workgroup per chunk), 2 the wide form
 * (17 .. 64 states: lane = state, one wave per chunk), 0 the row
 * form (one 16-lane DPP row per chunk, any trellis of <= 16 states), 1 the lane form (one lane per chunk, trellis compiled
 * in: the ARTM 16-state and PCM/FM 10-state designs of waveforms/cpm/multih, waveforms/cpm/pcmfm; bursts long enough for
 * its 64 chunks per wave to fill the chip, ~9e6 / ~6.5e6 calls); info4[1] = its LDS ring depth; info4[2] = calls per
 * chunk; info4[3] = warm-up calls.  Both forms make the same decisions, bit for bit (notes/cpm/cpm.md:100-140 is what both
 * implement).  Priced for the context's device (its compute-unit count) under the context's options
 * (WF_OPT_CPM_FORM, WF_OPT_CPM_CHUNK_CALLS): exactly what wf_cpm_viterbi_detect will launch.  No device work. */
int wf_cpm_detector_form(wf_ctx *ctx, const wf_cpm_detector_config *det, int64_t ncalls, int warmup, int *info4);
int wf_cpm_viterbi_detect(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs,
                          const double *d_rows_ri, int64_t ncalls, int warmup, uint8_t *d_decisions,
                          void *d_state, void *stream);

/* wf_cpm_mf_rows_c128 + wf_cpm_viterbi_detect in ONE launch (round 6): the detector reads the noisy SAMPLES — call k's window is
 * samples start0 + 8 k .. start0 + 8 k + 8, 128 new bytes per call where a 16-filter row is 256 — and runs the matched filters
 * itself, in the manner of examples/soqpsk_detection.py:134-156 (pulse-truncation templates) for the trellis of
 * notes/cpm/cpm.md:100-140.  The templates must pair off as exact conjugates, d_templates[c][nfilt-1-f] == conj(d_templates[c][f])
 * (checked on a host copy, WF_ERR_VALUE if not): each pair is formed from four real 9-tap sums, so the filter outputs equal
 * wf_cpm_mf_rows_c128's to rounding (another order of additions) and are bit for bit those of the link's paired one-kernel front
 * end (wf_cpm_link_config.fuse bit 6).  Serves the 16-filter, 16-state ARTM design at 8 samples per symbol, 9-tap templates,
 * start0 >= 0, on bursts of at least 6e6 calls (shorter ones are faster through rows and the row form): returns 1 — nothing launched,
 * not an error — otherwise, and the caller runs wf_cpm_mf_rows_c128 + wf_cpm_viterbi_detect.  Call k takes template column k % nh.
 * Decisions, d_state, warm-up, proof and repair as wf_cpm_viterbi_detect (the repairs rebuild the rows they need from the samples). */
int wf_cpm_viterbi_detect_samples(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs, const double *d_templates_ri,
                                  int nh, int nfilt, int ntm, const double *d_samples_ri, int64_t nsamp, int64_t start0, int sps,
                                  int64_t ncalls, int warmup, uint8_t *d_decisions, void *d_state, void *stream);

/* Symbol and bit errors of decided U against transmitted symbols alpha (int8):
 * d_counts[0] += #(U != (alpha + M - 1)/2), d_counts[1] += popcount(U ^ (alpha + M - 1)/2)
 * (the reference's mappers are natural binary: waveforms/cpm/multih/precoder.py:22-23). */
int wf_cpm_count_errors(wf_ctx *ctx, const uint8_t *d_decided_u, const int8_t *d_ref_alpha, int M, int64_t m,
                        int64_t *d_counts, void *stream);

/* ---- generic CPM soft output: max-log-MAP, per-bit LLRs, on the full-phase trellis -----------------------------------
 * The reduced designs (NC < p: ARTM_16, PCMFM_10) carry the phase index per survivor, which a backward recursion has no
 * survivor to carry; the soft output is therefore defined on the FULL-PHASE trellis of the same matched filters: a spec with
 * NC = p and S = p M^(Lp-1) <= 64 states (ARTM: the 64 states of ARTM_64, the same 16 filters per call as ARTM_16; PCM/FM:
 * 20 states).  State s = v + p c: v the phase index, c the Lp - 1 previous symbols.  A burst of N = ncalls calls (rows),
 * free start and free end; first_call = n0 is the global index of its first call.  Section k (global call n = n0 + k) has
 * the branches (s, u), u = 0 .. M-1, whose increment, end state, tilt, leaving-symbol modulation index and pre-start variant
 * are exactly those of cpm_oracle.c at call n:
 *   inc_k(s, u) = -fma(cos_r, Re Z_k[u + M c], sin_r * Im Z_k[u + M c]),  (cos_r, sin_r) = d_rot_cs[r],  r = (2 v - tilt(n)) mod 2p.
 * In float64 and in exactly this order of operations:
 *   ã_0 = 0;  a'_{k+1}(e) = min_{(s,u) -> e} (ã_k(s) + inc_k(s,u)) (+inf if no branch);   ã_{k+1} = a'_{k+1} - min_e a'_{k+1}(e)
 *   b̃_N = 0;  b'_k(s)     = min_u (inc_k(s,u) + b̃_{k+1}(e(s,u)));                         b̃_k     = b'_k - min_s b'_k(s)
 *   λ_{k,i} = min_{(s,u): bit_i(u) = 1} ((ã_k(s) + inc_k(s,u)) + b̃_{k+1}(e(s,u))) - min_{(s,u): bit_i(u) = 0} (the same)
 *   d_llr[lgM k + i] = λ_{k,i},   d_bits[lgM k + i] = λ_{k,i} < 0
 * Bit i of U is MSB first (the natural binary of the reference's mappers, waveforms/cpm/multih/precoder.py:22-23).  Section
 * k's input is the symbol whose filter column opens at call k (wf_cpm_viterbi_detect decides it at call k + D - 1), so
 * transmitted bit j pairs with λ[j].  λ > 0 favours bit 0; λ is in metric units, no scale baked in.
 * d_rows_ri: ncalls x M^Lp complex128, 16-byte aligned (the rows wf_cpm_viterbi_detect reads); det->D is ignored.  Each call
 * is a fresh burst.  Chunk-parallel with the proof and cascading repair of the hard detectors in BOTH directions, so the
 * result is bitwise the definition whatever `warmup` (calls, 0 = library default) and WF_OPT_CPM_SOFT_CHUNK_CALLS are;
 * WF_OPT_DET_REPAIR / WF_OPT_DET_FINAL_VERIFY act as for the hard detectors, repairs and unproven chunks (both directions)
 * are counted in wf_viterbi_repaired / wf_viterbi4_unmerged.  Scratch: the context's detector scratch
 * (wf_cpm_soft_geometry [3] bytes).  A NULL pointer, ncalls < 1, first_call < 0, warmup < 0, M not 2 / 4, nh not 1 / 2,
 * Lp outside 1 .. 3, NC != p or more than 64 states (ARTM_256): WF_ERR_VALUE before the context is touched. */
int wf_cpm_soft(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs, const double *d_rows_ri,
                int64_t ncalls, int64_t first_call, int warmup, double *d_llr, uint8_t *d_bits, void *stream);
/* What wf_cpm_soft launches for this burst on this context: h_geom[0] calls per chunk, [1] chunks, [2] warm-up calls used,
 * [3] scratch bytes.  Host only, no device work. */
int wf_cpm_soft_geometry(wf_ctx *ctx, const wf_cpm_detector_config *det, int64_t ncalls, int warmup, int64_t *h_geom);

/* wf_cpm_soft with a per-bit prior and EXTRINSIC per-bit output: the inner detector of iterative detection and decoding for
 * ARTM and PCM/FM.  Everything of wf_cpm_soft holds unchanged (full-phase spec with NC = p and at most 64 states, rows,
 * first_call, "transmitted bit j pairs with λ[j]", warm-up, chunk-parallel proof and cascading repair in both directions,
 * WF_OPT_CPM_SOFT_CHUNK_CALLS, WF_OPT_DET_REPAIR / WF_OPT_DET_FINAL_VERIFY, counters, scratch: wf_cpm_soft_geometry
 * describes this call too) with, in float64 and in exactly this order of operations, lgM = log2 M, bit i of u MSB first:
 *   π_{k,i}     = apriori_scale * (double)d_apriori[lgM k + i]                  (0 when d_apriori is NULL)
 *   Π_k(u)      = the sum of π_{k,i} over the bits i of u that are 1            (M = 4, u = 3: ONE addition π_{k,0} + π_{k,1})
 *   inc'_k(s,u) = inc_k(s,u) + Π_k(u) when u != 0, inc_k(s,u) when u = 0        (one float64 addition)
 *   ã, b̃: the recursions of wf_cpm_soft with inc' in place of inc
 *   x_{k,i}(s,u) = inc_k(s,u) + π_{k,j} when u has another bit j != i and that bit is 1, inc_k(s,u) otherwise
 *                  (M = 2: always inc_k(s,u); M = 4: bit 0 takes π_{k,1} on u = 1, 3 and bit 1 takes π_{k,0} on u = 2, 3)
 *   λᵉ_{k,i}    = min_{(s,u): bit_i(u) = 1} ((ã_k(s) + x_{k,i}(s,u)) + b̃_{k+1}(e(s,u))) - min_{(s,u): bit_i(u) = 0} (the same)
 *   d_ext[lgM k + i]  = λᵉ_{k,i},    d_bits[lgM k + i] = (λᵉ_{k,i} + π_{k,i}) < 0
 * A bit's own prior is never added into its own output (so none is subtracted); the prior of the other bit of the same
 * quaternary symbol is: the output is extrinsic per BIT, which is what a binary decoder needs.  For M = 2 this is the rule
 * of wf_viterbi4_soft_apriori.  π > 0 favours bit 0, as λ does.  d_apriori: lgM * ncalls float32, 4-byte aligned, indexed as
 * d_llr is (a decoder writes the next prior of codewords sent back to back at offset 0, stride n_tx).  With d_apriori NULL
 * the result is bitwise wf_cpm_soft's (and so it is for a prior of zeros of either sign: see below).
 * Why the order in which a machine takes the minima does not matter although inc' may be negative or -0: a normalised metric
 * ã, b̃ is x - min x over the states, which is >= +0 and never -0 (x - x = +0 in round-to-nearest; every state of the
 * full-phase trellis has exactly M entering and M leaving branches, so min x is finite and no state is ever +inf).  A sum with
 * an operand that is not -0 is not -0.  Every operand of a min is such a sum: ã_k(s) + inc', inc' + b̃_{k+1}(e), (ã_k(s) + x)
 * + b̃_{k+1}(e).  So no operand of a min is -0, equal operands are bitwise equal, and the result does not depend on the order.
 * An implementation may carry +inf for the lanes of a wave that hold no state: +inf plus a finite increment is +inf, never
 * the smaller operand and never NaN.  A prior of -0 gives π = -0 or +0 by the sign of apriori_scale, Π(3) = ±0, and
 * inc + (±0) differs from inc at most in the sign of a zero, which the next sum with ã or b̃ removes: zeros of either sign
 * are exactly "no prior".  Rows must be finite and every π_{k,i} and Π_k(3) finite in float64 (finite float32 priors and a
 * scale below 1e269 in magnitude guarantee it).  apriori_scale not finite, a prior that is not 4-byte aligned, or any
 * argument wf_cpm_soft refuses: WF_ERR_VALUE before the context is touched. */
int wf_cpm_soft_apriori(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs, const double *d_rows_ri,
                        int64_t ncalls, int64_t first_call, int warmup, const float *d_apriori, double apriori_scale,
                        double *d_ext, uint8_t *d_bits, void *stream);

/* ---- LDPC codes: systematic encoder and layered normalized min-sum decoder ------------------------------------------
 * A code is an opaque handle made once on the host.  H has n variables and m checks, numbered in LAYER order: check c's
 * edges are h_edge_var[h_check_ptr[c] .. h_check_ptr[c+1]) (table order), layer l holds checks h_layer_ptr[l] ..
 * h_layer_ptr[l+1].  Transmitted position t (0 .. n_tx-1) carries variable h_tx_var[t]: this one table is the bit
 * interleaver and the puncturing map (a variable it does not name is punctured).  h_info_var: the k information
 * variables, in message order; h_parity_gen: (n - k) rows of ceil(k / 64) words, row r for the r-th NON-information
 * variable in increasing order, bit i of word w (LSB first) multiplying message bit 64 w + i (parity = A u over GF(2));
 * NULL makes a decode-only code.  Checked on the host before any device memory is touched (WF_ERR_VALUE): 2 <= n <= 32768,
 * every check degree 2 .. 32, no variable twice in a check or in two checks of one layer, tx_var a bijection onto the
 * variables it names, info_var distinct and in range.  The tables are uploaded into device memory the handle owns
 * (synchronous); wf_ldpc_code_free releases it (synchronous). */
typedef struct wf_ldpc_code wf_ldpc_code;
int wf_ldpc_code_create(wf_ctx *ctx, int32_t n, int32_t m, const int32_t *h_check_ptr, const int32_t *h_edge_var,
                        int32_t nlayers, const int32_t *h_layer_ptr, int32_t n_tx, const int32_t *h_tx_var, int32_t k,
                        const int32_t *h_info_var, const uint64_t *h_parity_gen, wf_ldpc_code **out);
int wf_ldpc_code_free(wf_ldpc_code *code);
/* d_info: ncw x k bits (u8 0 / 1) -> d_tx: ncw x n_tx bits in transmit order (codeword b, position t = variable
 * tx_var[t]).  Decode-only code: WF_ERR_VALUE. */
int wf_ldpc_encode(wf_ctx *ctx, const wf_ldpc_code *code, const uint8_t *d_info, int64_t ncw, uint8_t *d_tx, void *stream);
/* Codeword b's LLR for transmitted position t is d_llr[b n_tx + t], λ > 0 favouring bit 0 (as the soft detectors give it;
 * the caller aligns by offsetting the pointer: for wf_viterbi4_soft, transmitted bit j is λ_{j+1}).  Per codeword, in
 * float32 and in exactly this order:
 *   L_v = (float)(scale * λ[src v]) (product in float64, then rounded); L_v = 0 for a punctured v; R_e = 0.
 *   Iteration 0: x̂_v = [L_v < 0]; if H x̂ = 0 the codeword is done with iters = 0.
 *   For t = 1 .. max_iter, for each layer in order, for each check c of the layer, edges e in table order:
 *     T_e = L_{v_e} - R_e
 *     m1 = min |T_e|, e1 = the first e attaining it (strict <), m2 = min over e != e1 of |T_e|, S = XOR of [T_e < 0]
 *     R_e = (float)(alpha * (e == e1 ? m2 : m1)), negated when S XOR [T_e < 0]
 *     L_{v_e} = T_e + R_e
 *   After each full iteration x̂ = [L < 0]; if H x̂ = 0 the codeword stops with iters = t.  Otherwise iters = max_iter
 *   and the codeword is not converged.  A codeword that has stopped is never updated again.
 * Outputs (each may be NULL): d_info_bits ncw x k (x̂ at the information variables), d_post ncw x n (L, by variable),
 * d_iters ncw.  With d_ref_info (ncw x k bits), d_counts[0..3] are ADDED: information bit errors, codewords with any
 * information bit error, codewords not converged, iterations summed.  Asynchronous on `stream`; the check state of a code
 * too large for LDS lives in the context's detector scratch (wf_ldpc_decode_geometry).  A NULL code / ctx / d_llr,
 * ncw < 1, max_iter outside 1 .. 10000, scale or alpha not finite and positive, d_ref_info without d_counts: WF_ERR_VALUE. */
int wf_ldpc_decode(wf_ctx *ctx, const wf_ldpc_code *code, const double *d_llr, int64_t ncw, double scale, float alpha,
                   int max_iter, uint8_t *d_info_bits, float *d_post, int32_t *d_iters,
                   const uint8_t *d_ref_info, int64_t *d_counts, void *stream);
/* What wf_ldpc_decode launches for ncw codewords: h_geom[0] check-state form (0: LDS, 1: context scratch), [1] codewords
 * per workgroup G, [2] workgroups per launch (the scratch form decodes a longer batch in several launches), [3] dynamic
 * LDS bytes per workgroup, [4] scratch bytes.  Host only. */
int wf_ldpc_decode_geometry(wf_ctx *ctx, const wf_ldpc_code *code, int64_t ncw, int64_t *h_geom);
/* wf_ldpc_decode with a per-codeword freeze state and an extrinsic output: the outer decoder of iterative detection and
 * decoding, called once per outer pass.  d_state: ncw bytes, in and out (0 = open, 1 = frozen).  Per codeword b:
 *   state 1 on entry: NOTHING of the codeword is read or written (d_info_bits, d_ext, d_post, d_iters and the state keep
 *     what an earlier call left) and it costs no decoding work.
 *   state 0: decoded exactly as wf_ldpc_decode defines (same float32 order, cold start R = 0, iteration 0 is the syndrome
 *     of the input).  d_iters[b] is INCREASED by the iterations used (max_iter when not converged).  If the codeword
 *     stopped with H x̂ = 0 (at any iteration 0 .. max_iter): state <- 1 and d_ext[b ext_stride + t] = x̂_{v_t} ? -ext_sat :
 *     +ext_sat.  Otherwise d_ext[b ext_stride + t] = min(max(L_{v_t} - Lch_{v_t}, -ext_clip), +ext_clip) with
 *     Lch_v = (float)(scale * λ) as the decoder loaded it and the subtraction in float32 (v_t = tx_var[t]).
 * A punctured variable has no d_ext entry.  ext_stride >= n_tx lets the call write straight into a burst's prior buffer
 * (wf_viterbi4_soft_apriori: d_ext = prior + 1, ext_stride = n_tx for codewords sent back to back).  d_info_bits, d_post
 * and d_iters may be NULL.  ext_clip > 0 (INFINITY: no clip), ext_sat finite and > 0, d_state and d_ext not NULL, and the
 * argument checks of wf_ldpc_decode: WF_ERR_VALUE otherwise.  Launch geometry: wf_ldpc_decode_geometry. */
int wf_ldpc_decode_ext(wf_ctx *ctx, const wf_ldpc_code *code, const double *d_llr, int64_t ncw, double scale, float alpha,
                       int max_iter, uint8_t *d_state, uint8_t *d_info_bits, float *d_post, int32_t *d_iters, float *d_ext,
                       int64_t ext_stride, float ext_clip, float ext_sat, void *stream);
/* The four counts of wf_ldpc_decode after the last outer pass, ADDED to d_counts[0..3]: information bit errors of
 * d_info_bits against d_ref_info (ncw x k bits each), codewords with one, codewords whose d_state is 0, d_iters summed. */
int wf_ldpc_count(wf_ctx *ctx, const wf_ldpc_code *code, const uint8_t *d_info_bits, const uint8_t *d_ref_info,
                  const uint8_t *d_state, const int32_t *d_iters, int64_t ncw, int64_t *d_counts, void *stream);

/* ---- Convolutional codes: terminated feed-forward encoder and exact max-log-MAP soft-in / soft-out decoder -----------------
 * (The reference has no coding layer; these entry points are defined here.)
 * Code: rate 1 / n_out, constraint length K = 3 .. 7, memory ν = K - 1, S = 2^ν <= 64 states, n_out = 2 .. 4.  The generators
 * h_gen[j] are K-bit masks whose bit ν (the MSB) taps the current input bit, so octal 171 / 133 read in the usual way.  Every
 * generator must have bit ν and bit 0 set: then every code bit takes both values on branches of the terminated trellis that lie
 * on a path, no -inf - (-inf) arises and every output below is finite.  No output is inverted.
 * Trellis: the message u_0 .. u_{k-1} is followed by ν zero tail bits, T = k + ν steps.  With s_0 = 0, step i has
 *   reg = (u_i << ν) | s_i,   c_{i,j} = parity(reg & g_j),   s_{i+1} = reg >> 1,
 * variable v = n_out i + j carries c_{i,j}, N = n_out T <= 32768.  Transmitted position t (0 .. n_tx-1) carries variable
 * h_tx_var[t]: this one table is the bit interleaver and the puncturing map, exactly as for the LDPC codes (a variable it does
 * not name is punctured).  Checked on the host before any device memory is touched (WF_ERR_VALUE): K, n_out, the generators'
 * end taps, k >= 1, N, 1 <= n_tx <= N, tx_var distinct and in range.  The tables are uploaded into device memory the handle
 * owns (synchronous); wf_conv_code_free releases it (synchronous). */
typedef struct wf_conv_code wf_conv_code;
int wf_conv_code_create(wf_ctx *ctx, int32_t K, int32_t n_out, const uint32_t *h_gen, int32_t k, int32_t n_tx, const int32_t *h_tx_var,
                        wf_conv_code **out);
int wf_conv_code_free(wf_conv_code *code);
/* d_info: ncw x k bits (u8 0 / 1) -> d_tx: ncw x n_tx bits in transmit order (codeword b, position t = variable tx_var[t]). */
int wf_conv_encode(wf_ctx *ctx, const wf_conv_code *code, const uint8_t *d_info, int64_t ncw, uint8_t *d_tx, void *stream);
/* Max-log-MAP over the whole block (no window), per codeword, in float32 and in exactly this order.  Codeword b's channel value
 * for transmitted position t is d_llr[b n_tx + t]; d_info_prior (ncw x k float32, or NULL) is the prior A_i of message bit i.
 * λ, A and the outputs Λ, P, ext all follow one convention: positive favours bit 0.
 *   L_v = (float)(scale * λ[src v]) (product in float64, then rounded); L_v = 0 for a punctured v; A_i = 0 when the pointer is NULL.
 *   Branch (s, u) of step i: γ starts as (u ? -A_i : +0); then, for j = 0 .. n_out-1 in this order, γ = γ - L_{n_out i + j} where
 *   c_{i,j} = 1 on the branch.  Only u = 0 exists for i >= k.
 *   α_0(0) = 0, every other α_0 = -INFINITY;   α_{i+1}(s') = max over the branches into s' of (α_i(s) + γ)
 *   β_T(0) = 0, every other β_T = -INFINITY;   β_i(s)     = max over u of (γ + β_{i+1}(s'))
 *   No normalisation.  Per branch V = (α_i(s) + γ) + β_{i+1}(s').
 *   Λ_i = max_{u = 0} V - max_{u = 1} V  (i < k);  the information bit is [Λ_i < 0]
 *   P_v = max_{c_{i,j} = 0} V - max_{c_{i,j} = 1} V
 *   d_ext[b ext_stride + t] = min(max(P_v - L_v, -ext_clip), +ext_clip), v = tx_var[t]   (a punctured variable has no entry)
 * A max never meets -0 (α and β start from +0 or -INFINITY, and a sum is -0 only when both operands are), so equal operands are
 * bitwise equal and the order in which a machine takes a max does not matter; the sums are taken as written.  An
 * implementation may keep α at checkpoints and recompute it (the same operations on the same operands); it may not window.
 * Inputs (λ, A) must be finite, with |L| and |A| small enough that no sum overflows: this is not checked on the device.
 * Outputs (each may be NULL): d_info_bits ncw x k, d_info_post ncw x k (Λ), d_ext as above (ext_stride >= n_tx lets the call
 * write straight into a burst's prior buffer; ext_clip > 0, INFINITY: no clip).  With d_ref_info (ncw x k bits), d_counts[0..1]
 * are ADDED: information bit errors, codewords with any.  Asynchronous on `stream`; the checkpoints live in the context's
 * detector scratch (wf_conv_siso_geometry).  A NULL code / ctx / d_llr, ncw < 1, scale not finite and positive, d_ext with
 * ext_stride < n_tx or ext_clip not > 0, d_ref_info without d_counts, a misaligned pointer: WF_ERR_VALUE.
 * Parallelism: a codeword is serial in its T steps (the order above is the definition), so a call has ncw S lanes of work:
 * lane = state, 64 / S codewords per wave. */
int wf_conv_siso(wf_ctx *ctx, const wf_conv_code *code, const double *d_llr, int64_t ncw, double scale, const float *d_info_prior,
                 uint8_t *d_info_bits, float *d_info_post, float *d_ext, int64_t ext_stride, float ext_clip,
                 const uint8_t *d_ref_info, int64_t *d_counts, void *stream);
/* What wf_conv_siso launches for ncw codewords: h_geom[0] codewords per wave (64 / S), [1] waves, [2] checkpoint spacing C in
 * steps, [3] LDS bytes per wave, [4] scratch bytes.  Host only. */
int wf_conv_siso_geometry(wf_ctx *ctx, const wf_conv_code *code, int64_t ncw, int64_t *h_geom);

/* ---- Turbo codes: two terminated RSC constituents, an interleaver, and a max-log-MAP decoder of all half-iterations ----------
 * (The reference has no coding layer; these entry points are defined here.)
 * Constituent: a recursive systematic convolutional code of constraint length K = 3 .. 5, memory ν = K - 1, S = 2^ν <= 16 states.
 * The feedback mask fb and the n_par = 1 .. 3 parity generators h_gen[0 .. n_par-1] (g_1 .. g_npar below) are K-bit masks whose
 * bit ν (the MSB) taps the current register input, so octal 13 / 15 read in the usual way.  Every mask must have bit ν and bit 0
 * set, and g_j != fb.  With f(s) = parity(s & (fb & (S - 1))), s_0 = 0 and T = k + ν steps:
 *   i < k:  a_i = u_i ^ f(s_i);      i >= k (the tail):  a_i = 0, so the tail bit sent is u_i = f(s_i) and the register empties;
 *   reg = (a_i << ν) | s_i,   c_{i,0} = a_i ^ f(s_i) = u_i = parity(reg & fb),   c_{i,j} = parity(reg & g_j),   s_{i+1} = reg >> 1,
 * m = 1 + n_par outputs per step.
 * Turbo code: constituent 1 encodes u_0 .. u_{k-1}, constituent 2 encodes u_π(0) .. u_π(k-1), π = h_perm, any bijection of
 * 0 .. k-1; both are terminated on their own.  Variable v = 2m i + j is output j of constituent 1 at step i, v = 2m i + m + j
 * output j of constituent 2, N = 2m T <= 32768.  Transmitted position t (0 .. n_tx-1) carries variable h_tx_var[t]: this one
 * table is the puncturing map and the channel interleaver, exactly as for the other codes.  (The usual choice sends every
 * variable except constituent 2's systematic output at the steps i < k.)  Checked on the host before any device memory is
 * touched (WF_ERR_VALUE): K, n_par, the masks' end taps, g_j != fb, k >= 1, N, π a bijection, 1 <= n_tx <= N, tx_var distinct
 * and in range.  π, its inverse, var -> src and tx_var are uploaded into device memory the handle owns (synchronous);
 * wf_turbo_code_free releases it (synchronous). */
typedef struct wf_turbo_code wf_turbo_code;
int wf_turbo_code_create(wf_ctx *ctx, int32_t K, int32_t n_par, uint32_t fb, const uint32_t *h_gen, int32_t k, const int32_t *h_perm,
                         int32_t n_tx, const int32_t *h_tx_var, wf_turbo_code **out);
int wf_turbo_code_free(wf_turbo_code *code);
/* d_info: ncw x k bits (u8 0 / 1) -> d_tx: ncw x n_tx bits in transmit order (codeword b, position t = variable tx_var[t]). */
int wf_turbo_encode(wf_ctx *ctx, const wf_turbo_code *code, const uint8_t *d_info, int64_t ncw, uint8_t *d_tx, void *stream);
/* The turbo decoder: half_iters = H (1 .. 64) max-log-MAP half-iterations per codeword in ONE call, in float32 and in exactly
 * this order.  Positive favours bit 0 everywhere.
 * Channel values: L_v = (float)(scale * λ[src v]) (product in float64, then rounded), L_v = 0 for a punctured v.  Ls1_i is L of
 * constituent 1's systematic variable at step i.  For i < k constituent 2's systematic value is Ls2_i = Ls1_π(i): it is COPIED,
 * whether or not constituent 2's own systematic variable is transmitted, and if that variable is transmitted its own L is
 * ignored by the decoding for i < k (it is only subtracted in that variable's own d_ext entry).  For i >= k each constituent
 * uses its own tail values.
 * SISO(c, A) of constituent c with the prior A_0 .. A_{k-1}: γ of branch (s, a) at step i starts as (u ? -A_i : +0) with
 * u = a ^ f(s) for i < k, and as +0 for i >= k; then, for j = 0 .. m-1 in this order, γ = γ - L_{c,i,j} where the branch's code
 * bit j is 1.  α, β, their boundary values and "no normalisation" are wf_conv_siso's, with only a = 0 for i >= k:
 *   α_0(0) = 0, every other α_0 = -INFINITY;   α_{i+1}(s') = max over the branches into s' of (α_i(s) + γ)
 *   β_T(0) = 0, every other β_T = -INFINITY;   β_i(s)     = max over a of (γ + β_{i+1}(s'))
 *   V = (α_i(s) + γ) + β_{i+1}(s');   P_{i,j} = max_{c_j = 0} V - max_{c_j = 1} V;   Λ_i = max_{u = 0} V - max_{u = 1} V = P_{i,0}  (i < k)
 * (Λ groups the branches by u, not by a.)  Every P is finite except that of a tail bit which is 0 in every codeword (k < ν
 * only): that one is +INFINITY.
 * Half-iterations h = 1 .. H.  Before the first, A1 = 0, or d_a1 (ncw x k float32, in and out) when given.
 *   odd h:   Λ1 = SISO(1, A1);  E1_i = ext_scale * ((Λ1_i - A1_i) - Ls1_i), the two subtractions and the product each rounded to
 *            float32;  A2_i = E1_π(i).
 *   even h:  Λ2 = SISO(2, A2);  E2_i = ext_scale * ((Λ2_i - A2_i) - Ls2_i);  A1_π(i) = E2_i.
 * Decision after an odd last half-iteration: x̂_i = [Λ1_i < 0] and post_i = Λ1_i; after an even one x̂_π(i) = [Λ2_i < 0] and
 * post_π(i) = Λ2_i.
 * Stop rule (early_stop != 0): after an even h, a codeword with [Λ2_i < 0] == [Λ1_π(i) < 0] for all i stops, iters = h / 2.  A
 * stopped codeword is never updated again: its outputs (d_a1 included) are those of its stopping half-iteration.  Otherwise
 * iters = ceil(H / 2).
 * d_ext[b ext_stride + t] (H even only), at the codeword's last half-iteration, v = tx_var[t]: for constituent 1's systematic
 * variable at i < k, X = (Λ2 deinterleaved)_i - Ls1_i; for every other variable X = P_{i,j} - L_v from the last SISO of its
 * constituent; the entry is min(max(X, -ext_clip), +ext_clip).  A punctured variable has no entry; ext_stride >= n_tx lets the
 * call write straight into a burst's prior buffer.
 * Outputs (each may be NULL): d_info_bits ncw x k, d_info_post ncw x k, d_iters ncw (int32), d_ext, d_a1 (A1 as the last
 * half-iteration left it).  With d_ref_info (ncw x k bits), d_counts[0..2] are ADDED: information bit errors, codewords with any,
 * half-iterations run summed over the codewords.  Inputs must be finite and small enough that no sum overflows (not checked on
 * the device).  A NULL code / ctx / d_llr, ncw < 1, scale or ext_scale not finite and positive, H outside 1 .. 64, d_ext with an
 * odd H, ext_stride < n_tx or ext_clip not > 0, d_ref_info without d_counts, a misaligned pointer, a code of another device:
 * WF_ERR_VALUE.  Asynchronous on `stream`, one launch for all half-iterations (several only for a batch whose scratch would
 * pass the cap): lane = state, 64 / S codewords per wave in lockstep; A1, A2, constituent 1's decisions and the α checkpoints
 * live in the context's detector scratch (wf_turbo_decode_geometry), nothing synchronises with the host. */
int wf_turbo_decode(wf_ctx *ctx, const wf_turbo_code *code, const double *d_llr, int64_t ncw, double scale, float ext_scale,
                    int32_t half_iters, int32_t early_stop, float *d_a1, uint8_t *d_info_bits, float *d_info_post, int32_t *d_iters,
                    float *d_ext, int64_t ext_stride, float ext_clip, const uint8_t *d_ref_info, int64_t *d_counts, void *stream);
/* What wf_turbo_decode launches for ncw codewords: h_geom[0] codewords per wave (64 / S), [1] waves, [2] checkpoint spacing C in
 * steps, [3] LDS bytes per wave, [4] scratch bytes.  Host only. */
int wf_turbo_decode_geometry(wf_ctx *ctx, const wf_turbo_code *code, int64_t ncw, int64_t *h_geom);

/* ---- Reed-Solomon codes over GF(2^8): systematic encoder and bounded-distance decoders, symbol-interleaved -------------------
 * (The reference has no coding layer; these entry points are defined here.)
 * Field: GF(2^8) = GF(2)[x] / prim(x), prim a 9-bit mask (bit 8 set; CCSDS: 0x187); a symbol is a byte whose bit i is the
 * coefficient of x^i, α is the class of x.  prim must be primitive: α has period 255.
 * Code: RS(n, k), 2t = n - k, t = 1 .. 16, n <= 255, k >= 1.  With β = α^step, gcd(step, 255) = 1, 1 <= step <= 254, and
 * 0 <= fcr <= 254, the generator is g(x) = Π_{i=0}^{2t-1} (x - β^(fcr+i)).  CCSDS (255, 223): step 11, fcr 112; CCSDS (255, 239):
 * step 11, fcr 120 (both generators are palindromic; their x^1 coefficients are 91 and 165).  The conventional code: prim 0x11d,
 * fcr 0, step 1.  n < 255 is the shortened code: 255 - n leading message symbols are zero and are never sent.
 * Codeword: c_0 .. c_{n-1}, c_0 sent first; as a polynomial c(x) = Σ c_i x^(n-1-i), so c_0 is the highest coefficient.  Encoding
 * is systematic: c_0 .. c_{k-1} are the message, c_k .. c_{n-1} the remainder of m(x) x^(2t) by g(x), highest coefficient first.
 * A word is a codeword exactly when its syndromes S_j = r(β^(fcr+j)), j = 0 .. 2t-1, are all zero.
 * Interleaving to depth I = 1 .. 8: a frame is n I transmitted symbols; the symbol at position p belongs to codeword p mod I
 * at index p div I.  A message frame is k I symbols laid out the same way.  Codeword b I + c is codeword c of frame b.
 * Bit form: bits = 0: one symbol per byte; bits = 1: one bit per byte (u8 0 / 1, only bit 0 is read), eight per symbol, most
 * significant bit first (the form wf_conv_encode reads and wf_conv_siso writes).
 * Checked on the host before the context or any device memory is touched (WF_ERR_VALUE): prim of degree 8 and primitive,
 * gcd(step, 255) = 1, and every range above.  The field tables are uploaded into device memory the handle owns (synchronous);
 * wf_rs_code_free releases it (synchronous). */
typedef struct wf_rs_code wf_rs_code;
int wf_rs_code_create(wf_ctx *ctx, int32_t prim, int32_t fcr, int32_t step, int32_t n, int32_t k, int32_t depth, wf_rs_code **out);
int wf_rs_code_free(wf_rs_code *code);
/* d_msg: nframes message frames (k I symbols each) -> d_tx: nframes frames (n I symbols each), both in the bit form `bits`.
 * The buffers must not overlap.  NULL pointer, nframes < 1, bits outside {0, 1}: WF_ERR_VALUE.  Asynchronous on `stream`. */
int wf_rs_encode(wf_ctx *ctx, const wf_rs_code *code, const uint8_t *d_msg, int64_t nframes, int32_t bits, uint8_t *d_tx, void *stream);
/* The decoder's result is defined by its outcome, not by an algorithm.  For each received word r of the (possibly shortened)
 * code, errors only:
 *   if a codeword c of that code lies within Hamming distance t of r, counted in symbols, it is unique: the output is c's
 *   message and status = d(r, c) = 0 .. t;  otherwise the output is r's own message symbols unchanged and status = -1.
 * (So a locator with a root at one of the 255 - n virtual positions is a failure, as is a locator of degree above t or one whose
 * number of roots among the n positions differs from its degree.)  Erasures: wf_rs_decode_erasures below.
 * d_rx: nframes frames -> d_msg_out: nframes message frames, d_status (int32 per codeword, b I + c; may be NULL).  With d_ref_msg
 * (nframes message frames) these are ADDED to d_counts[0..4] (int64): [0] message bit errors after decoding, [1] codewords
 * wrong after decoding, [2] codewords with status -1, [3] symbols corrected summed over the successful codewords, [4] frames
 * with any wrong codeword.  Miscorrections are [1] - [2].  d_msg_out must not overlap d_rx (a frame's message lies where other
 * workgroups may still be reading their input) or d_ref_msg.  NULL ctx / code / d_rx / d_msg_out, nframes < 1, d_ref_msg without
 * d_counts, bits outside {0, 1}, a misaligned d_status or d_counts: WF_ERR_VALUE.  Asynchronous on `stream`; nothing
 * synchronises with the host.  One workgroup per frame, one wave per codeword (wf_rs_decode_geometry). */
int wf_rs_decode(wf_ctx *ctx, const wf_rs_code *code, const uint8_t *d_rx, int64_t nframes, int32_t bits, uint8_t *d_msg_out,
                 int32_t *d_status, const uint8_t *d_ref_msg, int64_t *d_counts, void *stream);
/* What wf_rs_decode launches for nframes frames: h_geom[0] waves (codewords) per workgroup = I, [1] workgroups, [2] launches,
 * [3] LDS bytes per workgroup, [4] threads per workgroup (64 I).  Host only. */
int wf_rs_decode_geometry(wf_ctx *ctx, const wf_rs_code *code, int64_t nframes, int64_t *h_geom);
/* Errors and erasures, again defined by the outcome.  d_erase: nframes x n I bytes in SYMBOL form whatever `bits` is, laid out
 * like the frame, nonzero = erased.  For a received word r of the (possibly shortened) code, let E be the set of its f erased
 * positions among its n real positions.
 *   If f > 2t: the output is r's own message symbols unchanged and status = -1.
 *   Otherwise, if a codeword c of that code exists with 2 |{i not in E : c_i != r_i}| + f <= 2t, it is unique (two such
 *   codewords would differ outside E in at most (2t - f) / 2 + (2t - f) / 2 = 2t - f places, while the code punctured at E has
 *   minimum distance 2t + 1 - f): the output is c's message and status = e = |{i not in E : c_i != r_i}|, the number of
 *   positions OUTSIDE E that changed (an erased symbol that was received right or wrong counts in f only).
 *   Otherwise the output is r's own message symbols unchanged and status = -1.
 * The bytes received at erased positions decide nothing: the status, and on success the whole output, are the same for any two
 * inputs that differ only there.  (On a failure the output is the received message as it came, erased positions included:
 * that copy is the only use of those bytes.)  A candidate with a root at one of the 255 - n virtual positions is a failure, as
 * before.  With no position erased the outputs are exactly those of wf_rs_decode.
 * Buffers, d_status, alignment and the refusals are those of wf_rs_decode, and a NULL d_erase is refused too (WF_ERR_VALUE before
 * any launch).  d_counts has SIX entries: [0..4] as in wf_rs_decode ([3] adds the status, the errors outside E), [5] erasures
 * filled: f summed over the successful codewords.  Asynchronous on `stream`, nothing synchronises with the host; the geometry
 * is wf_rs_decode's: one workgroup per frame, one wave per codeword, one launch. */
int wf_rs_decode_erasures(wf_ctx *ctx, const wf_rs_code *code, const uint8_t *d_rx, const uint8_t *d_erase, int64_t nframes, int32_t bits,
                          uint8_t *d_msg_out, int32_t *d_status, const uint8_t *d_ref_msg, int64_t *d_counts, void *stream);
/* The rule that turns the inner decoder's soft output into erasures.  d_post: nframes x 8 n I float32 (4-byte aligned), the Λ
 * of wf_conv_siso (d_info_post) for frames in bit form, finite.  A symbol's reliability is ρ = min over its eight bits of |Λ|.
 * Per codeword the erased symbols are the at most f_max symbols of smallest ρ among those with ρ < below; of two symbols with
 * equal ρ the one with the smaller index in its codeword goes first.  d_erase (nframes x n I bytes, the form
 * wf_rs_decode_erasures reads) is written whole: 1 = erased, 0 = not.  f_max = 0 marks nothing.  NULL ctx / code / d_post /
 * d_erase, nframes < 1, f_max outside 0 .. 2t, below not finite, a misaligned d_post: WF_ERR_VALUE before any launch.
 * Asynchronous on `stream`; one workgroup per frame, one wave per codeword. */
int wf_rs_mark_erasures(wf_ctx *ctx, const wf_rs_code *code, const float *d_post, int64_t nframes, int32_t f_max, float below,
                        uint8_t *d_erase, void *stream);

/* ---- Framed coded links: attached sync marker, randomiser, soft frame search ------------------------------------------
 * (The reference has no coding or framing layer; these entry points are defined here.)
 * Frame: L marker bits (1 <= L <= 64) followed by the n_tx transmitted bits of one codeword, bit t exclusive-ored with
 * pn[t], t counted from the start of the codeword; period P = L + n_tx.  The marker is the low L bits of `marker`, sent MSB
 * first: marker bit i = (marker >> (L - 1 - i)) & 1.  It is not randomised.  d_pn: n_tx bytes (0 / 1) in device memory,
 * NULL = no randomiser; the package's own sequence is pn[0..7] = 1, pn[n+8] = pn[n] ^ pn[n+3] ^ pn[n+5] ^ pn[n+7]
 * (waveforms_amd/encoding/framing.py), the ABI is not tied to it.
 * wf_frame_build (transmit side): d_out[b P + i] = marker bit i (i < L), d_out[b P + L + t] = (d_tx[b n_tx + t] ^ pn[t]) & 1,
 * for b < ncw: ncw x P bytes. */
int wf_frame_build(wf_ctx *ctx, const uint8_t *d_tx, int64_t ncw, int32_t n_tx, uint64_t marker, int32_t L, const uint8_t *d_pn,
                   uint8_t *d_out, void *stream);
/* Soft search of the frame offset and polarity of a burst.  d_llr: nllr float64 λ, λ > 0 favouring bit 0, finite.  With
 * s_i = +1 where marker bit i is 0 and -1 where it is 1 (s_i λ flips the sign bit: no product is rounded), in float64, every
 * sum started from +0 and taken in exactly this order:
 *   C(t) = sum_{i = 0 .. L-1} s_i λ[t + i],  A(t) = sum_{i = 0 .. L-1} |λ[t + i]|          (i increasing)
 *   M+(t) = C(t) - A(t),   M-(t) = (-C(t)) - A(t)
 *   F = (nllr - L) div P frames;  slice j holds the frames f = 32 j .. min(32 j + 32, F) - 1
 *   S±(j, p) = sum of M±(p + f P) over the frames of slice j (f increasing);  G±(p) = sum_j S±(j, p) (j increasing), p < P
 * M+ <= 0 is minus twice the summed |λ| of the positions that disagree with the marker; M- the same for the inverted stream.
 * The lock is the maximum of the 2P values; ties go to + before -, then to the smallest p.  d_lock (32 bytes, 8-byte
 * aligned) receives { int64 p̂, int64 σ (+1, or -1 for the inverted stream), double best value, double the maximum of the
 * other 2P - 1 values } (best - other is the lock's margin); d_folded, if not NULL, the 2P values, G+(0 .. P-1) then
 * G-(0 .. P-1).  Nothing is returned to the host.  The slice sums ((ceil(F / 32) + 1) x 2P doubles) live in the context's
 * detector scratch, as the detectors' chunk records do: the call follows a detector on the same stream and context.
 * L outside 1 .. 64, P <= L or P > 2^23, F < 1, a NULL ctx / d_llr / d_lock, a pointer not 8-byte aligned: WF_ERR_VALUE
 * before the context is touched. */
int wf_frame_search(wf_ctx *ctx, const double *d_llr, int64_t nllr, uint64_t marker, int32_t L, int64_t P, void *d_lock,
                    double *d_folded, void *stream);
/* Deframe: the decoder's input from a located burst.  The lock record is READ FROM DEVICE MEMORY (no host round trip); with
 * r_t = 1 - 2 pn[t] and P = L + n_tx:
 *   d_out[b n_tx + t] = σ r_t λ[p̂ + b P + L + t]   for b < ncw, t < n_tx   (sign flips; a position at or beyond nllr gives +0)
 * d_out: ncw x n_tx float64, what wf_ldpc_decode / wf_ldpc_decode_ext read.  Alignment with a detector is by pointer offset,
 * for the search, the gather and the scatter alike: d_llr = llr + 1 and d_prior = prior + 1 behind wf_viterbi4_soft, offset 0
 * behind wf_cpm_soft. */
int wf_frame_gather(wf_ctx *ctx, const double *d_llr, int64_t nllr, const void *d_lock, int32_t L, int32_t n_tx, const uint8_t *d_pn,
                    int64_t ncw, double *d_out, void *stream);
/* Reframe: the decoder's extrinsic output (wf_ldpc_decode_ext's d_ext, float32) into a detector's prior buffer:
 *   d_prior[p̂ + b P + L + t] = σ r_t d_ext[b ext_stride + t]     for b < ncw, t < n_tx
 *   d_prior[p̂ + b P + i]     = σ s_i marker_prior                for i < L; marker_prior = 0 leaves these positions alone
 * A position at or beyond nprior is skipped; everything else in the buffer is left as it was.  The marker is a run of known
 * bits: a saturated marker_prior hands it to the detector on every later pass.  ext_stride < n_tx, marker_prior not finite,
 * L outside 1 .. 64, a NULL pointer (d_pn may be NULL): WF_ERR_VALUE before the context is touched. */
int wf_frame_scatter(wf_ctx *ctx, const float *d_ext, int64_t ext_stride, const void *d_lock, uint64_t marker, int32_t L, int32_t n_tx,
                     const uint8_t *d_pn, int64_t ncw, float marker_prior, float *d_prior, int64_t nprior, void *stream);

/* ---- Carrier phase and frequency: the impairment and a feed-forward, decision-directed recovery ------------------------
 * (The reference has no synchroniser; these entry points are defined here.  waveforms_amd/sync/carrier.py restates each in
 * numpy: carrier_offset_host, map_branch_host, carrier_stat_host, carrier_track_host, derotate_host.)
 * wf_carrier_offset_c128, the impairment at sample rate: out_k = in_k exp(j φ_k), in float64 and in this order:
 *   t = nu * (double)(first_index + k)   (turns; nu in cycles per sample);   f = t - floor(t)   (exact)
 *   φ_k = theta0 + (2π * f)              (one product, one sum);             out_k = in_k (cos φ_k + j sin φ_k)
 * so a sample index of 1e9 loses no phase beyond the rounding of t itself.  In-place allowed.  n < 1, first_index < 0,
 * first_index + n > 2^53, theta0 or nu not finite, a NULL pointer or samples not 16-byte aligned: WF_ERR_VALUE before the
 * context is touched. */
int wf_carrier_offset_c128(wf_ctx *ctx, const double *d_in_ri, int64_t n, double theta0, double nu, int64_t first_index,
                           double *d_out_ri, void *stream);
/* wf_viterbi4_soft on 48-byte rows (the packed rows drop the quadrature components the statistic below reads) with one more
 * output per row: d_branch[k] = the branch b* of column k % 2 with the smallest
 *   T_k(b) = (ã_k(start b) + inc_k(b)) + b̃_{k+1}(end b),
 * b = 2 start + lsb the index in the column's list order (end = (start & 1) + 2 lsb in column 0, (start & 2) + lsb in
 * column 1), ties to the smallest b: the section-k branch of a maximum-likelihood path.  d_llr and d_bits are BITWISE
 * wf_viterbi4_soft's: the first launch, the proof and the repairs are the same code, only the last launch differs.
 * Everything else (alignment, warm-up, chunking, options, counters, scratch) as wf_viterbi4_soft; a NULL d_branch or any
 * argument wf_viterbi4_soft refuses: WF_ERR_VALUE before the context is touched. */
int wf_viterbi4_soft_branch(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int differential, int warmup, double *d_llr,
                            uint8_t *d_bits, uint8_t *d_branch, void *stream);
/* The decision-directed phase statistic per window of W rows (W a multiple of 64, 64 .. 8192); nwin = ceil(ncalls / W).
 * q_k = state_exp_term[start b*_k] * z_k[idx(out b*_k)] = x_k + j y_k with state_exp_term = [+j, -1, +1, -j]: x and y are
 * signed components of z (no product is rounded); x_k = inc_k(b*_k) is the metric of the decided branch, so a coherent
 * burst has X << 0 and a rotation of the rows by θ turns (X, Y) by θ.  d_stat[w] = (X_w, Y_w), float64, in exactly this order:
 *   p_l = sum_i x[w W + 64 i + l]   (i increasing, started from +0; rows at or beyond ncalls contribute nothing), l < 64
 *   for d = 32, 16, .., 1:  p_l = p_l + p_{l+d}  for l < d;          X_w = p_0;  Y_w likewise from y.
 * d_branch: ncalls bytes, 0 .. 7 (wf_viterbi4_soft_branch's).  W outside its range, ncalls < 1, a NULL pointer, rows not
 * 16-byte or d_stat not 8-byte aligned: WF_ERR_VALUE before the context is touched. */
int wf_carrier_stat(wf_ctx *ctx, const double *d_rows, const uint8_t *d_branch, int64_t ncalls, int W, double *d_stat, void *stream);
/* Statistics -> a phase trajectory, on the device.  d_stat_h: H x nwin x 2 float64, the statistics of H passes over the
 * whole burst whose rows were derotated by h π / H first (wf_rows_derotate, phase0 = h π / H), h < H; H = 1: a refinement.
 *   h*_w = argmin_h X_{h,w} (ties to the smallest h);  ψ_w = ((double)h*_w * π) / H + atan2(-Y, -X) at h*_w
 *   u_0 = ψ_0;  u_w = u_{w-1} + wrap(ψ_w - ψ_{w-1}),  wrap(x) = x - π ceil(x / π - 1/2) in (-π/2, π/2]   (w increasing)
 *   d_phase[w] = (sum of u_j, j = max(0, w - r) .. min(nwin - 1, w + r), j increasing, from +0) / the number of terms, r = (span - 1) / 2
 * The unwrapping is modulo π: the trellis is symmetric under π, and a framed link's polarity σ absorbs what remains.
 * d_phase: nwin float64, d_choice: nwin bytes (h*).  The u_w pass through the context's detector scratch.  atan2 is the
 * device library's and the running sum u_w is taken as a blocked scan (segment sums, then offsets): this stage agrees with a
 * host statement to rounding - within 8 * 2^-52 * max(1, |phase|) * nwin - not bitwise.  H outside 1 .. 256, nwin < 1, span
 * even or < 1, a NULL pointer, a pointer not 8-byte aligned: WF_ERR_VALUE before the context is touched. */
int wf_carrier_track(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double *d_phase, uint8_t *d_choice, void *stream);
/* Derotate 48-byte rows: z_k <- z_k exp(-j (phase0 + φ_k)), all three values of a row.  φ_k interpolates d_phase linearly
 * between the window centres w W + (W - 1) / 2 and is held flat outside the first and the last one:
 *   t = ((double)k - (W - 1) / 2) / W;   t <= 0: φ = phase[0];   t >= nwin - 1: φ = phase[nwin - 1];
 *   otherwise w = floor(t), f = t - w, φ = phase[w] + (f * (phase[w + 1] - phase[w]))        (each operation rounded once)
 * d_phase NULL: φ = 0, a constant rotation (W and nwin are then not read).  In-place allowed.  ncalls < 1, phase0 not
 * finite, W outside 64 .. 8192 in steps of 64 or nwin < 1 (with d_phase), a NULL ctx / d_rows / d_out, rows not 16-byte or
 * d_phase not 8-byte aligned: WF_ERR_VALUE before the context is touched. */
int wf_rows_derotate(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int W, const double *d_phase, int64_t nwin, double phase0,
                     double *d_out, void *stream);

/* ---- The same recovery for the generic CPM detectors (ARTM, PCM/FM) -----------------------------------------------------
 * (waveforms_amd/sync/carrier_cpm.py restates each in numpy: cpm_map_branch_host, carrier_stat_terms_host, and
 * carrier_track_host / interpolate_phase_host of carrier.py with a period.)  The full-phase trellis is exactly symmetric
 * under a rotation of the rows by P = 2π / p: it moves every state's phase index v by one and leaves the input symbols
 * alone, so the estimate is modulo P and the ambiguity never reaches the data.
 * wf_cpm_soft_branch is wf_cpm_soft with two more outputs per call.  With T_k(s,u) = (ã_k(s) + inc_k(s,u)) + b̃_{k+1}(e(s,u)),
 * the operand of wf_cpm_soft's λ minima:
 *   d_branch[k] = b* = M s* + u*, the (s, u) with the smallest T_k, ties to the smallest b (S M <= 256: a byte)
 *   d_term[2k], d_term[2k+1] = (x_k, y_k), the components of q_k = -Z_k[f] e^{-j φ_r} on that branch, f = u* + M c(s*), r of s*:
 *     x_k = inc_k(s*, u*)   (the metric term itself),    y_k = -fma(cos_r, Im Z_k[f], -(sin_r * Re Z_k[f]))
 * Every T is >= +0 and never -0 (the argument above), so equal T are bitwise equal and the tie rule is exact in any order of
 * comparison.  A rotation of the rows by θ turns q_k by θ: the angle of -Σ q_k over a window estimates θ.  A coarse
 * hypothesis is this call with a rotated table: entry r = (cos, sin)(π r / p + θ_h) detects the rows derotated by θ_h without
 * a pass over them.  d_llr and d_bits are BITWISE wf_cpm_soft's: the bounds, proof and repair launches are the same code,
 * only the last launch differs.  d_branch: ncalls bytes; d_term: 2 ncalls float64, 16-byte aligned, or NULL (not written).
 * Everything else (alignment, warm-up, chunking, options, counters, scratch) as wf_cpm_soft; a NULL d_branch, a d_term not
 * 16-byte aligned or any argument wf_cpm_soft refuses: WF_ERR_VALUE before the context is touched. */
int wf_cpm_soft_branch(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs, const double *d_rows_ri,
                       int64_t ncalls, int64_t first_call, int warmup, double *d_llr, uint8_t *d_bits, uint8_t *d_branch,
                       double *d_term, void *stream);
/* wf_carrier_stat from the terms wf_cpm_soft_branch wrote: d_stat[w] = (X_w, Y_w) from x = d_term[2k], y = d_term[2k+1] in
 * exactly wf_carrier_stat's order of additions (64 lane partials from +0, i increasing, then d = 32 .. 1).  W outside its
 * range, ncalls < 1, a NULL pointer, terms not 16-byte or d_stat not 8-byte aligned: WF_ERR_VALUE before the context is touched. */
int wf_carrier_stat_terms(wf_ctx *ctx, const double *d_term, int64_t ncalls, int W, double *d_stat, void *stream);
/* wf_carrier_track with `period` in place of π, in ψ_w = ((double)h*_w * period) / H + atan2(-Y, -X) and in
 * wrap(x) = x - period ceil(x / period - 1/2); hypothesis h derotated by h period / H.  wf_carrier_track is this with
 * period = π (one kernel), and the same bound against a host statement holds.  period not finite or outside (0, 2π], or any
 * argument wf_carrier_track refuses: WF_ERR_VALUE before the context is touched. */
int wf_carrier_track_mod(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double period, double *d_phase,
                         uint8_t *d_choice, void *stream);
/* wf_rows_derotate for rows of nvals complex128 (1 .. 64; ARTM 16, PCM/FM 4): the same φ_k, the same order of operations, all
 * nvals values of row k; wf_rows_derotate is nvals = 3 (one kernel).  nvals outside 1 .. 64 or any argument wf_rows_derotate
 * refuses: WF_ERR_VALUE before the context is touched. */
int wf_rows_derotate_n(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int nvals, int W, const double *d_phase, int64_t nwin,
                       double phase0, double *d_out, void *stream);

/* ---- Symbol timing for the SOQPSK-TG receiver: the impairment, a resampling matched-filter bank and a feed-forward recovery --
 * (The reference has no synchroniser; these entry points are defined here.  waveforms_amd/sync/timing.py restates each in
 * numpy: lagrange_host, timing_offset_host, mf_bank_resample_host, timing_track_host, timing_refine_host.)  All float64.
 * The cubic Lagrange weights of the nodes -1, 0, 1, 2 at a fraction μ in [0, 1):
 *   c_-1 = -μ(μ-1)(μ-2)/6    c_0 = (μ+1)(μ-1)(μ-2)/2    c_1 = -(μ+1)μ(μ-2)/2    c_2 = (μ+1)μ(μ-1)/6
 * (each the products left to right, then the division).
 * wf_timing_offset_c128, the impairment at sample rate: the signal read at n + t_n,
 *   t_n = tau0 + (eps * (double)(first_index + n))   (the product rounded, then the sum);   b_n = floor(t_n);   μ_n = t_n - b_n   (exact)
 *   out_n = Σ_{i = -1 .. 2} c_i(μ_n) in[n + b_n + i],   a sample outside [0, n) counting as zero
 * so (0, 0) returns the input.  OUT OF PLACE only: an output that overlaps the input is refused.  n < 1, first_index < 0,
 * first_index + n > 2^53, tau0 or eps not finite, a NULL pointer, samples not 16-byte aligned or overlapping: WF_ERR_VALUE
 * before anything is launched. */
int wf_timing_offset_c128(wf_ctx *ctx, const double *d_in_ri, int64_t n, double tau0, double eps, int64_t first_index,
                          double *d_out_ri, void *stream);
/* Matched-filter rows at fractional, time-varying instants, in one pass over the samples.  With v_f(n) the full-rate value of
 * wf_mf_bank_c128 (np.convolve(r, taps[f], "same")[n] for 0 <= n < nsamp, 0 elsewhere), row k < ncols samples the bank at
 *   T_k = first + k step + tau0 + τ_k:   t = tau0 + τ_k;   B_k = first + k step + floor(t);   μ_k = t - floor(t)   (exact)
 *   d_out[k][f] = Σ_{i = -1 .. 2} c_i(μ_k) v_f(B_k + i),    f < 3
 * τ_k interpolates d_tau[nwin] exactly as wf_rows_derotate interpolates its phase (linear between the window centres
 * w W + (W - 1) / 2, flat outside the first and the last; each operation rounded once); d_tau NULL: τ_k = 0 (W and nwin are
 * then not read).  A t that is not finite (or at or beyond 2^62) writes a zero row.  Any finite trajectory is served: rows
 * may fall before sample 0 or behind the last one, and neighbouring rows may be any distance apart.  The full-rate bank is
 * never formed: by linearity the kernel interpolates each of the ntaps samples a row needs once and runs the three filters on
 * them, so the result agrees with the definition to the rounding of a sum of ntaps + 4 terms, not bitwise.  d_taps_ri:
 * 3 x ntaps complex128; d_out_ri: ncols 48-byte rows.  nfilt other than 3, ntaps even or outside 1 .. 255, step outside
 * 1 .. 64, nsamp or ncols outside 1 .. 2^40, |first| > 2^40, tau0 not finite, (with d_tau) W outside 64 .. 8192 in steps of 64
 * or nwin < 1, a NULL ctx / samples / taps / out, data not 16-byte or d_tau not 8-byte aligned: WF_ERR_VALUE before the context
 * is touched. */
int wf_mf_bank_resample_c128(wf_ctx *ctx, const double *d_r_ri, int64_t nsamp, const double *d_taps_ri, int nfilt, int ntaps,
                             int64_t first, int step, int64_t ncols, int W, const double *d_tau, int64_t nwin, double tau0,
                             double *d_out_ri, void *stream);
/* The guarded vertex of the parabola through (-1, a), (0, b), (1, c): den = (a - b) + (c - b); V = 0.5 (a - c) / den if
 * den > 0, otherwise 0 (three points that are not strictly convex have no minimum to offer), then clamped to ±lim.
 * wf_timing_track: statistics -> a timing trajectory in samples.  d_stat_h: H x nwin x 2 float64 as wf_carrier_stat writes it
 * (only X is read), pass h taken at the instant s_h = (h * (period / H)) - period / 2, 3 <= H <= 64.  Per window
 *   i = argmin_h X_{h,w} (ties to the smallest h);   V = vertex(X_{(i-1) mod H}, X_i, X_{(i+1) mod H}), lim = 1/2
 *   ψ_w = s_i + ((period / H) * V)
 *   u_0 = ψ_0;  u_w = u_{w-1} + wrap(ψ_w - ψ_{w-1}),  wrap(x) = x - period ceil(x / period - 1/2)      (w increasing)
 *   d_tau[w] = the centred mean of u over span windows, exactly as wf_carrier_track takes it
 * d_choice: nwin bytes (i).  The running sum is a blocked scan through the context's detector scratch, as wf_carrier_track's:
 * within (nwin + span + 8) 2^-53 (|ψ_0| + Σ |wrapped steps|) of a host statement.  H outside 3 .. 64, nwin < 1, span even or
 * < 1, period not finite or not positive, a NULL pointer, a pointer not 8-byte aligned: WF_ERR_VALUE before the context is touched. */
int wf_timing_track(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double period, double *d_tau,
                    uint8_t *d_choice, void *stream);
/* A refinement: d_stat3 is 3 x nwin x 2, taken at τ - δ, τ, τ + δ.  d_more[w] = the centred mean over span windows of
 * δ * vertex(X_{0,w}, X_{1,w}, X_{2,w}) with lim = 1; no unwrapping.  The caller adds d_more to τ.  nwin < 1, span even or < 1,
 * delta not finite or not positive, a NULL pointer, a pointer not 8-byte aligned: WF_ERR_VALUE before the context is touched. */
int wf_timing_refine(wf_ctx *ctx, const double *d_stat3, int64_t nwin, int span, double delta, double *d_more, void *stream);

/* ---- The anchored unwrapping: both trackers without cycle slips (opt-in; the entry points above are untouched) --------------
 * (waveforms_amd/sync/_stages.py restates it in numpy: anchored_unwrap.)  The running unwrap of wf_timing_track and
 * wf_carrier_track follows every ψ_w: one window whose estimate errs by more than P/2 minus the drift leaves the trajectory a
 * whole period off for the rest of the burst.  The anchored form smooths on the circle first and unwraps second.  With ψ_w
 * (w < nwin) what the tracker forms before unwrapping, P its period, K = anchor (odd, 3 .. 1023), D = max_drift (ψ's unit per
 * window, 0 <= D < P/2) and ρ = reject (0 < ρ <= P/2):
 *   1. z_w = exp(j 2π frac(ψ_w / P))   (the quotient, t - floor(t), the product with 2π, then cos and sin); ψ_w not finite: z_w = 0
 *   2. candidates f_i = i / (4K) cycles per window, |i| <= n = ceil(((double)(4K) * D) / P); segments of K windows starting at
 *      s = 0, 2K, 4K, .. (the last may be short):
 *        score_i = Σ_segments |Σ_{j < K} z_{s+j} exp(-j 2π ((i j) mod 4K) / (4K))|²
 *      the inner sum with j increasing from +0, |.|² as re re + im im, the segments added in increasing order from +0;
 *      f̂ = the first candidate of the largest score
 *   3. y_w = z_w exp(-j 2π ((î w) mod 4K) / (4K))   (i j and î w are reduced as integers: no angle grows with the burst)
 *      a_w = Σ y_j, j = max(0, w - K/2) .. min(nwin - 1, w + K/2) increasing, from +0 (K/2 rounded down);  α_w = atan2(Im a_w, Re a_w)
 *      (a window with no finite ψ within K/2 of it has a_w = +0 and α_w = 0: it has no anchor, and comes back marked)
 *      u = the running unwrap of α modulo 2π, exactly wf_carrier_track's u;   r_w = ((P / 2π) * u_w) + ((P * f̂) * (double)w)
 *   4. d_w = wrap(ψ_w - r_w) modulo P;  ψ'_w = r_w + d_w;  if ψ_w is not finite or |d_w| > ρ: ψ'_w = r_w and d_marks[w] = 1 (else 0)
 *   5. the output = the centred mean of ψ' over span windows, exactly as wf_carrier_track takes it;  d_drift[0] = P * f̂
 * nwin = 1: the output is ψ_0 (0 if it is not finite), d_drift[0] = 0.  Two launches: the drift search runs as a grid over
 * (segments, candidates) and writes per-segment scores, one workgroup adds them in segment order and does steps 3 to 5; z, ψ,
 * α and the scores (4 nwin + ceil(nwin / 2K) (2n + 1) float64) pass through the context's detector scratch.  sincos and atan2 are
 * the device library's and the complex products contract: the scores agree with the host statement to rounding, so f̂ and
 * the marks equal the host's wherever the host's best score leads and no |d_w| sits at ρ, and the output then agrees to the
 * rounding of its own magnitude (a few ulp of the largest |r_w|), as the plain entry point's.
 * wf_timing_track_anchored: ψ_w of wf_timing_track (H, period as there);  wf_carrier_track_anchored: ψ_w of wf_carrier_track_mod
 * (H, period as there; period = π is wf_carrier_track's).  d_drift: one float64; d_marks: nwin bytes.  anchor, max_drift or
 * reject outside the ranges above, nwin > 2^31, a NULL pointer, or any argument the plain entry point refuses: WF_ERR_VALUE
 * before the context is touched. */
int wf_timing_track_anchored(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double period, int anchor,
                             double max_drift, double reject, double *d_tau, uint8_t *d_choice, double *d_drift, uint8_t *d_marks,
                             void *stream);
int wf_carrier_track_anchored(wf_ctx *ctx, const double *d_stat_h, int H, int64_t nwin, int span, double period, int anchor,
                              double max_drift, double reject, double *d_phase, uint8_t *d_choice, double *d_drift, uint8_t *d_marks,
                              void *stream);

/* ---- Joint carrier and timing acquisition for the SOQPSK-TG receiver: all carrier hypotheses of a pass in one set of launches --
 * (waveforms_amd/sync/joint.py composes the search from the stages above; these two entry points stack its hypotheses.)
 * wf_rows_derotate_hyp: H rotated copies of ncalls 48-byte rows, d_out[h][k], h < H, k < stride (H stride rows in all):
 *   k < ncalls:   d_out[h][k] = d_rows[k] exp(-j ((double)h * π) / H), all three values of the row, BITWISE what
 *                 wf_rows_derotate writes with d_phase NULL and phase0 = ((double)h * π) / H (the same operations);
 *   otherwise:    zero rows (+0.0), so that wf_carrier_stat over the whole buffer with a W that divides stride is H x
 *                 (stride / W) x 2 and no window takes rows of two copies.
 * Every input row is read once.  OUT OF PLACE only.  H outside 1 .. 256, ncalls < 1, stride < ncalls or not a multiple of
 * 64, H stride beyond 2^40, a NULL pointer, rows not 16-byte aligned or an output that overlaps the input: WF_ERR_VALUE before
 * the context is touched. */
int wf_rows_derotate_hyp(wf_ctx *ctx, const double *d_rows, int64_t ncalls, int H, int64_t stride, double *d_out, void *stream);
/* wf_viterbi4_soft (d_branch NULL) or wf_viterbi4_soft_branch (d_branch given: 48-byte rows only) over nseg INDEPENDENT trellis
 * segments of one buffer, in ONE set of launches (bounds, two fix-ups, last).  Segment s < nseg is rows s stride .. s stride +
 * seglen - 1, detected from a free start and to a free end as a burst of its own: its λ, bits and branches are BITWISE what
 * the burst entry point gives for those rows alone, whatever warm-up and chunk length (no chunk crosses a segment, no warm-up
 * leaves one, a segment's first chunk starts exactly as chunk 0 of a burst does, and every other chunk start is proven or
 * repaired).  stride is even, so row k of the buffer is trellis column k % 2 in its segment too.  Outputs are addressed as the
 * rows are and hold nseg stride values each: those of the pad rows s stride + seglen .. (s + 1) stride - 1, which are never
 * read, are written as 0.  d_rows holds (nseg - 1) stride + seglen rows at least.  The chunk length is wf_viterbi4_soft's for a
 * burst of nseg seglen rows (WF_OPT_SOFT_CHUNK_CALLS); options, counters and scratch as wf_viterbi4_soft.  nseg < 1 or beyond
 * 2^20, seglen < 1, stride odd or < seglen, nseg stride beyond 2^40, a packed d_rows with a d_branch, or any argument
 * wf_viterbi4_soft refuses: WF_ERR_VALUE before the context is touched. */
int wf_viterbi4_soft_branch_segments(wf_ctx *ctx, const double *d_rows, int64_t nseg, int64_t seglen, int64_t stride, int row_bytes,
                                     int differential, int warmup, double *d_llr, uint8_t *d_bits, uint8_t *d_branch, void *stream);

/* ---- Symbol timing for the generic CPM chains (ARTM multi-h, PCM/FM) --------------------------------------------------------
 * (waveforms_amd/sync/timing_cpm.py restates each in numpy: cpm_mf_rows_resample_host, llr_stat_host; the trajectory stages
 * are wf_timing_track and wf_timing_refine above, untouched.)
 * wf_cpm_mf_rows_resample_c128: the rows of wf_cpm_mf_rows_c128 at fractional, time-varying instants, in one pass over the
 * samples.  Row n < ncalls is taken at start0 + n sps + t_n:
 *   t_n = tau0 + τ_n, τ_n interpolated from d_tau[nwin] exactly as wf_mf_bank_resample_c128 interpolates it (d_tau NULL: τ = 0,
 *   W and nwin are then not read);   b = floor(t_n);   μ = t_n - b   (exact);   c_i = the Lagrange weights above at μ
 *   x_n[k] = fma(c_2, r[g+2], fma(c_1, r[g+1], fma(c_0, r[g], c_-1 * r[g-1])))   per component,  g = start0 + n sps + b + k,  k < ntm,
 *            a sample outside [0, nsamp) counting as zero
 *   rows[n][f] = Σ_k x_n[k] conj(T[n % nh][f][k]),  k ascending from zr = zi = +0:
 *            zr = fma(x.re, t.re, fma(x.im, t.im, zr));   zi = fma(-x.re, t.im, fma(x.im, t.re, zi))
 * The order of operations is part of the definition: a C restatement with explicit fma() agrees BITWISE.  For a finite whole
 * t_n the weights are (-0, 1, 0, -0), x_n[k] = r[g], and the row EQUALS wf_cpm_mf_rows_c128's at start0 + t_n.  A t_n that is not
 * finite, or at or beyond 2^62 in magnitude, writes a zero row, and so does a row all of whose samples lie outside the burst.
 * Any finite trajectory is served: rows may fall before sample 0 or behind the end, and neighbouring rows may be any distance
 * apart (a tile of rows whose samples span more than the staged window reads them from global memory, with the same
 * arithmetic).  d_templates_ri: nh x nfilt x ntm complex128, the templates (not reversed, not conjugated); d_rows_ri:
 * ncalls x nfilt complex128.  nh outside {1, 2}, nfilt outside {2, 4, 8, 16, 64}, ntm outside 1 .. 257, sps outside 1 .. 256 (or
 * a combination whose tile does not fit LDS), nsamp or ncalls outside 1 .. 2^40, |start0| > 2^40, tau0 not finite, (with d_tau)
 * W outside 64 .. 8192 in steps of 64 or nwin < 1, a NULL ctx / samples / templates / rows, data not 16-byte or d_tau not
 * 8-byte aligned: WF_ERR_VALUE before the context is touched. */
int wf_cpm_mf_rows_resample_c128(wf_ctx *ctx, const double *d_r_ri, int64_t nsamp, const double *d_templates_ri, int nh, int nfilt,
                                 int ntm, int64_t start0, int sps, int64_t ncalls, int W, const double *d_tau, int64_t nwin,
                                 double tau0, double *d_rows_ri, void *stream);
/* What wf_cpm_mf_rows_resample_c128 launches for these shapes: h_geom[0] rows per tile (one workgroup serves a tile at a time),
 * [1] the most workgroups a launch has (bursts with more tiles walk them in a grid-stride loop), [2] bytes of LDS per workgroup.
 * Host only.  The shapes' refusals are wf_cpm_mf_rows_resample_c128's. */
int wf_cpm_mf_rows_resample_geometry(int nh, int nfilt, int ntm, int sps, int64_t *h_geom);
/* The timing statistic of the CPM chains: the summed LLR magnitude per window of W calls of bits_per_call values each (a wrong
 * sampling instant makes ambiguous decisions).  nwin = ceil(ncalls / W); window w holds the values
 * λ[bits_per_call W w .. min(bits_per_call W (w + 1), bits_per_call ncalls) - 1]; in exactly wf_carrier_stat's order of additions:
 *   p_l = sum_i |λ[base + 64 i + l]|   (i increasing, started from +0; indices beyond the window contribute nothing), l < 64
 *   for d = 32, 16, .., 1:  p_l = p_l + p_{l+d}  for l < d;      d_stat[2w] = -p_0;   d_stat[2w + 1] = +0
 * so wf_timing_track and wf_timing_refine take the table as it is (they read X only).  d_llr: bits_per_call ncalls float64 as
 * wf_cpm_soft writes them.  ncalls outside 1 .. 2^40, bits_per_call outside 1 .. 8, W outside 64 .. 8192 in steps of 64, a NULL
 * pointer, a pointer not 8-byte aligned: WF_ERR_VALUE before the context is touched. */
int wf_llr_stat(wf_ctx *ctx, const double *d_llr, int64_t ncalls, int bits_per_call, int W, double *d_stat, void *stream);

/* ---- Joint carrier and timing acquisition for the generic CPM chains: the hypotheses of a pass in one set of launches -------
 * (waveforms_amd/sync/joint_cpm.py composes the search from the stages above; this entry point stacks its detections.)
 * wf_cpm_soft_branch over nseg INDEPENDENT segments in ONE set of launches (bounds, per direction one verify and three repair
 * rounds, last).  Segment s < nseg is a burst of its own: seglen calls whose call indices start at first_call, from a free
 * start to a free end;
 *   its rows:    d_rows_ri + s row_stride rows (M^Lp complex128 each); row_stride = 0: every segment reads the same rows
 *   its table:   d_rot_cs + s rot_stride tables of 2p (cos, sin) pairs; rot_stride is 0 or 1
 *   its outputs: at call offset s out_stride - λ and bits lgM values per call, the branch one byte per call, the term two
 *                float64 per call (d_term NULL: not written); the outputs of the calls s out_stride + seglen ..
 *                (s + 1) out_stride - 1 are written as +0 / 0, so that wf_llr_stat and wf_carrier_stat_terms over all
 *                nseg out_stride calls with a W that divides out_stride give the nseg separate tables.
 * Every output of segment s is BITWISE what wf_cpm_soft_branch writes for those rows, that table and that first_call alone,
 * whatever the warm-up and the chunk length: no chunk crosses a segment, no warm-up leaves one, a segment's first and last chunk
 * start exactly as a burst's do, the proof chain of either direction never compares records of two segments, and every other
 * chunk start is proven or repaired.  Two uses: row_stride 0 with rot_stride 1 - Hc carrier hypotheses of one set of rows (a
 * CPM carrier hypothesis is a rotated table, not a pass over the rows) -, and row_stride >= seglen with rot_stride 0 - several
 * sets of rows under one table.  The chunk length is wf_cpm_soft's for a burst of nseg seglen calls
 * (WF_OPT_CPM_SOFT_CHUNK_CALLS); options and counters as wf_cpm_soft; scratch: wf_cpm_soft_segments_geometry [3] bytes.
 * nseg outside 1 .. 2^20, seglen < 1, row_stride neither 0 nor >= seglen, rot_stride outside {0, 1}, out_stride < seglen or
 * not a multiple of 64, nseg out_stride (or nseg row_stride, nseg seglen) beyond 2^40, or any argument wf_cpm_soft_branch
 * refuses: WF_ERR_VALUE before the context is touched. */
int wf_cpm_soft_branch_segments(wf_ctx *ctx, const wf_cpm_detector_config *det, const double *d_rot_cs, int64_t rot_stride,
                                const double *d_rows_ri, int64_t nseg, int64_t seglen, int64_t row_stride, int64_t out_stride,
                                int64_t first_call, int warmup, double *d_llr, uint8_t *d_bits, uint8_t *d_branch, double *d_term,
                                void *stream);
/* What wf_cpm_soft_branch_segments launches on this context: h_geom[0] calls per chunk, [1] chunks in all, [2] warm-up calls,
 * [3] bytes of scratch, [4] chunks per segment.  Host only. */
int wf_cpm_soft_segments_geometry(wf_ctx *ctx, const wf_cpm_detector_config *det, int64_t nseg, int64_t seglen, int warmup,
                                  int64_t *h_geom);

/* Device-resident link for these waveforms (one bench step / trial block):
 * PRBS -> mapper (wf_symbol_map kind) -> cpm_modulate -> *exp(-j pi/4) + AWGN -> matched-filter
 * rows -> detector -> error count over symbols [skip_head, ncalls - D].  Stage events as in
 * wf_link_run (slots: prbs, map, modulate, -, awgn, mfbank, viterbi, count). */
typedef struct {
    int64_t nsym;
    int sps;
    int degree;
    uint64_t mask, state, skip;
    int mapper_kind;          /* 1: MultiHSymbolMapper (2 bits/symbol), 2: PCMFMSymbolMapper       */
    wf_cpm_detector_config det;
    const double *d_h;        /* device: nh modulation indices K[i]/p as doubles                  */
    const double *d_pulse;    /* device: frequency pulse                                          */
    int ntaps;
    const double *d_templates; /* device: nh x M^Lp x (sps+1) complex128                           */
    const double *d_rot_cs;   /* device: 2p x (cos, sin)                                          */
    double sigma;
    uint64_t seed, stream_id;
    int warmup;
    int skip_head;            /* leading symbols excluded from the comparison (start transient)   */
    int event_slot;
    int fuse;                 /* bit 1: channel applied inside the matched-filter kernel;         */
                              /* bit 3 (with bit 1, sps 8, 4 or 16 filters): modulator + channel  */
                              /* + matched-filter rows in one kernel, no samples in HBM;          */
                              /* bit 4 (16): PRBS and mapper as two kernels (wf_lfsr_generate +   */
                              /* wf_symbol_map) instead of the link's one launch (same symbols);  */
                              /* bit 5 (32): as wf_link_config.fuse bit 5 — the detector and the  */
                              /* error count of a block on the context's side stream, beside the   */
                              /* next block's front end; two sets of intermediates in the         */
                              /* workspace; wf_link_join / wf_ctx_check before the counters are read; */
                              /* bit 6 (64, with bit 3; nf = 4 or 16 filters): the templates pair   */
                              /* off as exact conjugates, d_templates[c][nf-1-f] ==                */
                              /* conj(d_templates[c][f]) (a symmetric alphabet: the negated symbol */
                              /* pattern negates the phase) — CHECKED value for value on a host    */
                              /* copy the first time these pointers are seen on a context          */
                              /* (WF_ERR_VALUE if not so) — the one-kernel front end then forms     */
                              /* each pair from four real 9-tap sums (16 filters: 6 matrix          */
                              /* instructions per 16 symbols instead of 10; 4 filters: 18 multiply- */
                              /* adds per lane instead of 36); rows equal to rounding, not bitwise; */
                              /* bit 7 (128, with bits 1 and 6; 16 filters, sps 8, a burst the      */
                              /* detector's lane form takes): the front end stores the noisy        */
                              /* SAMPLES (128 B per symbol: cpm_modulate + the channel, one kernel) */
                              /* and the detector runs the matched filters itself                  */
                              /* (wf_cpm_viterbi_detect_samples): no rows in HBM, decisions bit for */
                              /* bit those of bits 1 + 3 + 6; ignored where it does not apply       */
                              /* (wf_cpm_link_form tells)                                          */
} wf_cpm_link_config;
int64_t wf_cpm_link_workspace_bytes(const wf_cpm_link_config *cfg);
int wf_cpm_link_run(wf_ctx *ctx, const wf_cpm_link_config *cfg, void *d_workspace, int64_t workspace_bytes,
                    int64_t *d_counts, int64_t *h_compared, void *stream);
/* info8 = {ncalls, start0, off(decisions), off(symbols alpha), off(signal), one_kernel (1: fuse bits 1 + 3 run modulator +
 * channel + filters as one kernel for this configuration), signal samples, off(rows)} */
int wf_cpm_link_layout(const wf_cpm_link_config *cfg, int64_t *info8);
/* What wf_cpm_link_run launches for this configuration on this context (its options and device): info4[0] = front end — 0:
 * modulator, channel and matched filters as separate kernels, 1: one kernel with rows out (fuse bits 1 + 3), 2: modulator +
 * channel in one kernel with SAMPLES out and the matched filters inside the detector (fuse bit 7) —, info4[1 .. 3] = the
 * detector's form, calls per chunk and warm-up calls as wf_cpm_detector_form reports them.  No device work. */
int wf_cpm_link_form(wf_ctx *ctx, const wf_cpm_link_config *cfg, int *info4);

/* Streaming form of the CPM link (the scheme of wf_link_stream_chunk for the waveforms of BASELINE configs[2]):
 * a stream of cfg->nsym symbols in chunks of chunk_symbols detector calls, HBM footprint of one chunk; chunk c
 * makes calls [c*B, (c+1)*B).  Neighbouring context is re-generated as a halo (PRBS leap-ahead, memoryless
 * mapper, counter-based noise, one modulator tile either side) or carried in d_state
 * (WF_CPM_STREAM_STATE_BYTES, zero-initialised: detector state + modulator phase carry).  Chunks must be
 * processed in order; decisions and counts equal wf_cpm_link_run over the whole stream.  chunk_symbols: a
 * multiple of one modulator tile (wf_mod_tile_geometry) and of 128, at least 4 halos; the configuration must be
 * one the one-kernel front end takes (fuse bits 1 + 3; wf_cpm_link_layout info8[5]).
 * wf_cpm_link_stream_layout: info8 = {calls in the chunk, first call index, off(decisions), off(symbols alpha),
 * global index of symbols[0], calls of the whole stream, symbols per modulator tile, off(rows)}. */
#define WF_CPM_STREAM_STATE_BYTES 20480
int64_t wf_cpm_link_stream_workspace_bytes(const wf_cpm_link_config *cfg, int64_t chunk_symbols);
int wf_cpm_link_stream_layout(const wf_cpm_link_config *cfg, int64_t chunk_symbols, int64_t chunk_index, int64_t *info8);
int wf_cpm_link_stream_chunk(wf_ctx *ctx, const wf_cpm_link_config *cfg, int64_t chunk_symbols, int64_t chunk_index,
                             void *d_state, void *d_workspace, int64_t workspace_bytes, int64_t *d_counts,
                             int64_t *h_compared, void *stream);
/* The same chunk in parts, for callers that pipeline consecutive chunks on two HIP streams (own workspace and own
 * wf_ctx per stream; wf_link_stream_chunk_phase's numbering): phases bit 0 = PRBS + mapper (depends on nothing),
 * bit 2 = modulator + channel + matched-filter rows (after this chunk's bit-0 part and the previous chunk's bit-2 part:
 * the phase carry in d_state), bit 1 = detector + error count (after this chunk's bit-2 part and the previous chunk's
 * bit-1 part: the detector carry).  7 = wf_cpm_link_stream_chunk.  Replaces, for a stream, the per-call chain of
 * waveforms/cpm/modulate.py:57-101 + waveforms/noise.py:8-32 + the build-defined detector of wf_cpm_viterbi_detect. */
int wf_cpm_link_stream_chunk_phase(wf_ctx *ctx, const wf_cpm_link_config *cfg, int64_t chunk_symbols, int64_t chunk_index,
                                   void *d_state, void *d_workspace, int64_t workspace_bytes, int64_t *d_counts,
                                   int64_t *h_compared, int phases, void *stream);

/* ---- Coarse carrier frequency acquisition for SOQPSK-TG: feed-forward, one pass over the noisy samples ------------------
 * (The reference has no synchroniser; these entry points are defined here.  waveforms_amd/sync/coarse.py restates each in
 * numpy: line_samples_host, line_spectra_host, coarse_estimate_host, correct_host.)
 * SOQPSK-TG is a CPM with h = 1/2: the square of the received signal carries two spectral lines at 2 nu ± (1 + eps) / (2 sps)
 * cycles per sample (nu the carrier offset, eps the clock drift).  Inputs: r_k, k < n, complex128; sps 2 .. 64; S = smooth,
 * 1 .. 1024; L = nfft, a power of two from 64 to 4096; R = search >= 1.
 * 1. Line samples.  y_k = Σ_{j < S} r_{k+j} (j increasing);  z_k = y_k²;  nb = (n - S + 1) / sps (integer division);
 *      u_σ[m] = Σ_{i < sps} z_{m sps + i} exp(jσπ ((m sps + i) mod 2 sps) / sps)   (i increasing),  m < nb,  σ ∈ {-1, +1}:
 *    σ = -1 brings the upper line down to 2 nu, σ = +1 the lower line up.  The 2 sps rotations are a table, exp(jπ q / sps).
 * 2. Line spectra.  nseg = nb / L (the tail is dropped; nseg < 1: WF_ERR_VALUE);
 *      P_σ[b] = Σ_{s < nseg} |FFT_L(w ⊙ u_σ[s L : (s + 1) L])[b]|²   in fftshift order (bin L/2 is frequency 0),
 *    w = d_window, L doubles (np.hanning(L) in the Python layer).  d_spectra = [P₋ | P₊], 2 L doubles.  Workgroup partials
 *    (d_scratch: wf_coarse_scratch_doubles(n, sps, nfft, smooth) doubles; -1 where the arguments would be refused) are added
 *    in a fixed order, with no floating-point atomics: two launches on the same input give the same bits.
 * 3. Estimate (wf_coarse_estimate).  T = P₋ + P₊;  i* = the first maximum of T over the bins R + 1 .. L - R - 2;  per line
 *    i_σ = the first maximum of P_σ over i* - R .. i* + R (a NaN never wins);  f_σ = i_σ + d with, on a, b, c = the natural
 *    logs of the bins i_σ - 1, i_σ, i_σ + 1,   d = ½ (a - c) / ((a - b) + (c - b)),   d = 0 where that denominator is not negative
 *    and finite or where any of the three bins is <= 0 or not finite.
 *      d_found[0] = nu  = ((f₋ + f₊) / 2 - L / 2) / (2 L sps)   cycles per sample
 *      d_found[1] = eps = (f₋ - f₊) / L       (a clock drift moves the two lines apart; reported, not used here)
 *      d_found[2] = T[i*],  d_found[3] = the mean of T: a lock indicator for the caller, nothing here thresholds them.
 *    search outside 1 .. L / 2 - 2: WF_ERR_VALUE.
 * 4. Correction (wf_carrier_offset_dev_c128).  out_k = in_k exp(j 2π frac(nu (first_index + k))) with nu = gain * d_nu[0] read
 *    from device memory (gain a host scalar: -1 removes the estimate): the operations of wf_carrier_offset_c128 with
 *    theta0 = 0 in the same order, so the result is BITWISE what that entry point gives for the same value passed from the host.
 *    In place (d_out_ri == d_in_ri) allowed; a partial overlap, or d_nu inside the output, is refused.
 * A NULL pointer, samples not 16-byte or doubles not 8-byte aligned, an output that overlaps an input or the scratch, n
 * outside 1 .. 2^40 (the correction: first_index + n <= 2^53), gain not finite: WF_ERR_VALUE before the context is touched. */
int64_t wf_coarse_scratch_doubles(int64_t n, int sps, int nfft, int smooth);
int wf_coarse_lines_c128(wf_ctx *ctx, const double *d_r_ri, int64_t n, int sps, int smooth, int nfft, const double *d_window,
                         double *d_scratch, double *d_spectra, void *stream);
int wf_coarse_estimate(wf_ctx *ctx, const double *d_spectra, int nfft, int sps, int search, double *d_found, void *stream);
int wf_carrier_offset_dev_c128(wf_ctx *ctx, const double *d_in_ri, int64_t n, const double *d_nu, double gain,
                               int64_t first_index, double *d_out_ri, void *stream);

/* ---- Multi-symbol noncoherent soft detector for PCM/FM (Osborne and Luntz) ------------------
 * (The reference has no such detector; the entry points are defined here.  waveforms_amd/viterbi/noncoherent.py restates them in
 * numpy: noncoherent_templates_host, noncoherent_soft_host.)
 * Per bit, N symbols of samples are correlated with the noise-free signal of every N-bit hypothesis and the correlation
 * MAGNITUDES are compared: no carrier phase is needed, and a frequency offset costs only what it turns within one window.
 * Inputs: r_k, k < n, complex128; N odd, 3 .. 7; K = N sps; c = (N - 1) / 2; the table T, complex128[2^N][K], row-major.
 * Table (built on the host and uploaded; any table is taken as it is).  Row p, sample k:
 *      T[p][k] = exp(j 2π h Σ_{i < N} a_i q[k + offset - i sps]),   a_i = 2 bit_{N-1-i}(p) - 1   (MSB first, as wf_cpm_soft
 *    numbers a symbol's bits),   q[m] = (Σ_{l <= m} pulse[l]) / sps, 0 for m < 0 and its last value behind the pulse:
 *    samples offset .. offset + K - 1 of the modulator's output for the N bits of p alone, without the initial phase and the
 *    channel's derotation (magnitudes do not see them).  0 <= offset <= sps.
 * Detector.  Bit j's window begins at sample w_j = start + (j - c) sps;  r_k = 0 for k outside [0, n);
 *      z_p = Σ_{k < K} r[w_j + k] conj(T[p][k])
 *      λ_j = max_{p: bit c of p is 0} |z_p| - max_{p: bit c of p is 1} |z_p|        d_llr[j]
 *      d_bits[j] = λ_j < 0
 *    λ > 0 favours bit 0 (the sign of wf_cpm_soft).  The magnitude, not its square: the max-log form of ln I0(2 |z| / N0).  An
 *    all-zero window gives λ = +0 and bit 0.  The host statement adds k increasing; the kernel runs the product on the fp64
 *    matrix cores as four real chains per hypothesis and joins them, so it agrees to rounding - |λ - λ_host| <=
 *    2 · 8 (K + 8) 2^-53 Σ_k |r[w_j + k]| - and not bit for bit.  Input is taken to be finite.
 * wf_noncoherent_geometry: h_geom[0] bits per tile (one workgroup), [1] workgroups launched for nbits, [2] LDS bytes each.
 * N other than 3, 5, 7, sps other than 4, 8, 10, 16, 20 (the kernel's instantiations), n or nbits outside 1 .. 2^40, |start| >
 * 2^40, a NULL pointer, samples or table not 16-byte or d_llr not 8-byte aligned, outputs that overlap each other or an input:
 * WF_ERR_VALUE before the context is touched. */
int wf_noncoherent_geometry(wf_ctx *ctx, int N, int sps, int64_t nbits, int64_t *h_geom);
int wf_noncoherent_soft_c128(wf_ctx *ctx, const double *d_received_ri, int64_t n, const double *d_templates_ri, int N, int sps,
                             int64_t start, int64_t nbits, double *d_llr, uint8_t *d_bits, void *stream);

/* ---- data products of the reference's plotting helpers (no plotting) ------------------
 * Welch PSD exactly as Axes.psd / matplotlib.mlab.psd evaluates the call of
 * waveforms/viz/psd.py:36-41 (window d_window of nfft doubles, np.hanning for the reference;
 * no overlap, no detrend, two-sided, not scaled by frequency): d_pxx[nfft] in fftshift order =
 * mean over the n // nfft segments of |FFT(window * scale * x)|^2 / wsum^2 (wsum = sum |window|).
 * nfft a power of two <= 4096; d_scratch holds wf_welch_scratch_doubles(n, nfft) doubles. */
int64_t wf_welch_scratch_doubles(int64_t n, int nfft);
int wf_welch_psd_c128(wf_ctx *ctx, const double *d_x_ri, int64_t n, int nfft, double scale, const double *d_window,
                      double wsum, double *d_scratch, double *d_pxx, void *stream);
/* Phase-tree traces (waveforms/viz/tree.py:64-70): per chunk of sps*modulo samples np.unwrap(np.angle)
 * minus `off`, or minus the chunk's first phase when use_first != 0.  d_out: (n / len) x len. */
int wf_phase_tree_f64(wf_ctx *ctx, const double *d_x_ri, int64_t n, int sps, int modulo, int use_first, double off,
                      double *d_out, void *stream);
/* Eye-diagram traces (waveforms/viz/eye.py:40-55): (n-1)/len traces of len+1 points, len = sps*modulo:
 * time axis (time - time[start]) + t_offset, real and imaginary planes.  BOTH d_time and d_x_ri must hold n elements. */
int wf_eye_traces_c128(wf_ctx *ctx, const double *d_time, const double *d_x_ri, int64_t n, int sps, int modulo,
                       double t_offset, double *d_t_out, double *d_re_out, double *d_im_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WFHIP_H */
