/*
 * tmhip.h — C-ABI of libtmhip.so, the MI355X (gfx950) implementation of
 * TmLibrary's corilla illumination-statistics path and its apply step.
 *
 * The reference (scottberry/TmLibrary) is pure Python and has no FFI; these
 * entry points are the boundary its Python classes would bind through
 * ctypes.  Each function names the reference interface it replaces.
 *
 * Conventions
 *   - Every int-returning function returns 0 on success and a negative
 *     errno-style code on failure; tmh_last_error() holds a thread-local
 *     message for the last failure on the calling thread.
 *   - "host" pointers are plain CPU memory owned by the caller; "dev"
 *     pointers are device (HBM) memory on the handle's device, owned by the
 *     caller unless stated otherwise.
 *   - stream arguments are hipStream_t passed as void*; NULL means the
 *     handle's own stream.  Host-pointer calls are synchronous on return.
 *   - A handle is not thread-safe; distinct handles may be used from
 *     distinct threads.  No callbacks.
 *   - Sites are contiguous [n_sites][height][width] uint16 images in site
 *     order (the order of batch['channel_image_files_ids'],
 *     tmlib/workflow/corilla/api.py:125-136).
 */
#ifndef TMHIP_H
#define TMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TMH_ABI_VERSION 9

#define TMH_OK 0
#define TMH_EINVAL (-22)  /* bad argument: maps to ValueError / TypeError */
#define TMH_ENOMEM (-12)  /* device or host allocation failed             */
#define TMH_EDEVICE (-5)  /* HIP runtime error                            */
#define TMH_ESTATE (-71)  /* call not valid in the handle's state         */

/* ---- library ---------------------------------------------------------- */
int tmh_abi_version(void);
const char* tmh_last_error(void);
int tmh_device_count(int* n);
int tmh_set_device(int device);
int tmh_synchronize(void* stream);

/* ---- illumination statistics ------------------------------------------
 * Replaces tmlib/workflow/corilla/stats.py:35-121 (OnlineStatistics):
 *   __init__(image_dimensions, decimals)  -> tmh_stats_create
 *   update(image, log_transform)           -> tmh_stats_update[_device]
 *   mean / std / var / percentiles         -> tmh_stats_finalize[_device]
 *
 * n_quantiles = 10**(decimals+2).  q_lo/q_hi/q_gamma are numpy 2.2.6's
 * linear-percentile sorted positions and weights for an image of
 * height*width pixels (previous/next index after the above/below-bound
 * substitution, gamma = virtual - previous), computed on the host so they
 * are bit-identical to np.percentile (stats.py:76).
 * lut_log10[65536] is the stats log transform of every uint16 value
 * (np.log10 with 0 -> 0, stats.py:79-85), built by the host's numpy.
 * batch_capacity is the number of sites the handle stages per launch for
 * host-pointer updates (device updates of any size are processed in
 * place).  flags: TMH_STATS_DEFERRED_PCT keeps every site's order
 * statistics on the device instead of folding them into the accumulator at
 * each update (needed for the multi-GPU percentile chain).
 */
typedef struct tmh_stats tmh_stats;

#define TMH_STATS_DEFERRED_PCT 1u
#define TMH_STATS_KEEP_SITE_HIST 2u /* keep per-site histograms (debug/parity) */
#define TMH_STATS_SERIAL 4u         /* no side stream: histogram after Welford */

int tmh_stats_create(int height, int width, int n_quantiles, const int64_t* q_lo,
                     const int64_t* q_hi, const double* q_gamma, const double* lut_log10,
                     int batch_capacity, unsigned flags, tmh_stats** out);
void tmh_stats_destroy(tmh_stats* h);
int tmh_stats_set_stream(tmh_stats* h, void* stream);
/* Start a new job on the handle (stats.py:53-62 state).  Also restores the
 * handle's zero-maintained histogram slabs if a fused pass was interrupted. */
int tmh_stats_reset(tmh_stats* h);

/* Options of a handle (results never depend on them).  The automatic
 * choices below come from the job's SITE PROBE: at the first Welford launch
 * after tmh_stats_reset, one small kernel samples 16,384 8-pixel groups
 * spread over the launch's first <= 64 sites, and the host waits for its
 * three counts (groups sampled, holding a value >= 4,096, >= 16,384) --
 * so that launch returns only once the probe has run on its stream.  Only
 * the chosen kernels are queued.  The choice assumes the first <= 64 sites
 * stand for the job: a job whose first sites are dark and later sites very
 * wide runs the narrow configurations, its wide values taking their global-
 * atomic path -- results identical, the pass slower (uniform 16-bit sites
 * that way: ~0.5 s per 3,456 sites, against ~36 ms chosen right;
 * test_gpu_parity.py dark_prefix_wide_tail).  Force a configuration
 * (TMH_OPT_FUSED_CONFIG) for such jobs.
 *   TMH_OPT_FUSED_CONFIG   (sites per unit, threads, LDS bins) of the fused
 *                          correct+histogram pass: 3 = (4, 512, 16384), 5 =
 *                          (4, 1024, 65536 u16 counters packed two sites to a
 *                          word).  -1 (default): from the probe -- 3; or 5
 *                          when >= 2% of the probed groups hold a value >=
 *                          4,096; or, when >= 33% hold a value >= 16,384
 *                          ("very wide" sites, e.g. uniform 16-bit data), the
 *                          pass runs without its histogram and a per-site
 *                          u16-pair LDS histogram pass (one more read) builds
 *                          them; 100 forces that form.  0, 1, 2 and 4 (one or
 *                          two sites per unit, 32,768 u32 bins: 17.7 against
 *                          16.0 ms on bright sites, common.h) were measured
 *                          slower and removed: TMH_EINVAL.
 *   TMH_OPT_WELFORD_PARTS  0 (default): automatic -- with the log transform,
 *                          a launch of >= 96 sites whose job probe found >=
 *                          10% of the groups holding a value >= 4,096 (bright
 *                          sites: the log10 pass is VALU-bound) runs the
 *                          16,384-entry LUT pass in 3 site parts (merged in
 *                          order), else one part; 1..4: that many parts where
 *                          the launch has >= 32 sites a part
 *   TMH_OPT_COPY_THREADS   1..64 (default 8): host threads of the pageable <->
 *                          pinned copies of the host-buffer entry points'
 *                          outputs (inputs go straight from the caller's) */
#define TMH_OPT_FUSED_CONFIG 1
#define TMH_OPT_WELFORD_PARTS 2
/* 3, 6 and 7 were TMH_OPT_TAIL_CHUNKS / TMH_OPT_PCT_TAIL / TMH_OPT_FUSED_EPOCHS
 * (percentile-tail variants measured slower than the default, removed); 5 was
 * TMH_OPT_HOST_STAGING (its other modes: a pinned input bounce slower than the
 * runtime's pageable path, and an unpinned output; never selected, removed) */
#define TMH_OPT_COPY_THREADS 4
int tmh_stats_set_option(tmh_stats* h, int option, int value);

/* update(image) for a run of sites.  zero_counts_out (host, n_sites, may be
 * NULL): per-site number of zero pixels, for the 'image contains zero
 * values' warning (stats.py:81-82).  Host sites move in chunks of the
 * handle's batch capacity through two device slots on a copy stream, so
 * chunk k's H2D overlaps chunk k-1's kernels; returns when all are done. */
int tmh_stats_update(tmh_stats* h, const uint16_t* host_sites, int64_t n_sites,
                     int log_transform, int64_t* zero_counts_out);
/* Stream contract of the device update entry points: on another stream than
 * the handle's, the work runs after everything already queued on the
 * handle's stream, and the handle's stream waits for it before any later work
 * on the handle (finalize, merge, ...), so results read on the handle's
 * stream are complete.  The wait is queued with the handle's next work (a
 * wait queued at once would hold up every stream sharing the handle stream's
 * hardware queue until the awaited pass ended): work a caller queues on the
 * handle's stream itself, outside this library, is not ordered after it --
 * order such work against the caller's stream, or synchronise. */
int tmh_stats_update_device(tmh_stats* h, const uint16_t* dev_sites, int64_t n_sites,
                            int log_transform, void* stream);
/* Per-site zero-pixel counts of the LAST CHUNK of the last update call: the
 * call's sites in chunks of 4,096, so for a call of <= 4,096 sites these are
 * its sites' counts (n <= that chunk's size, else TMH_EINVAL).  Copied to
 * host_out on `stream` after the handle's queued work (asynchronous for
 * pinned host_out). */
int tmh_stats_zero_counts(tmh_stats* h, int64_t* host_out, int64_t n, void* stream);

/* Split job pipeline (one read of the sites per pass):
 *   tmh_stats_update_welford_device  Welford only; the sites' percentile
 *                                    contributions are left pending
 *   tmh_correct_u16_hist_device      (below) corrects the SAME sites, in the
 *                                    same order, and builds their histograms
 *                                    from that read, completing the pending
 *                                    percentile state.
 * Results are identical to tmh_stats_update_device + tmh_correct_u16_device. */
int tmh_stats_update_welford_device(tmh_stats* h, const uint16_t* dev_sites, int64_t n_sites,
                                    int log_transform, void* stream);

/* The job's site probe (see the options above), queued now on `stream`
 * without waiting for it: the first Welford launch of the job then only
 * waits for the probe's counts.  A caller running several jobs on several
 * streams (a rank's channels) queues every job's probe first, so that no
 * launch waits for another job's kernels to drain before its probe can run.
 * Optional: a job not probed this way is probed by its first Welford launch.
 * Stream: the probe reads only the sites and its counts go to the host, so
 * it is ordered after `stream`'s queued work alone (the sites must be ready
 * there; NULL: the handle's stream) and nothing of the handle waits for it:
 * on a stream of its own it runs as soon as the sites are, whatever the
 * handle still has queued (the previous job's merges and tails).  Call it
 * after tmh_stats_reset. */
int tmh_stats_probe_device(tmh_stats* h, const uint16_t* dev_sites, int64_t n_sites,
                           void* stream);
int tmh_stats_probe_blocks_device(tmh_stats* h, const uint16_t* const* dev_blocks, int block_shift,
                                  int64_t n_sites, void* stream);

/* Blocked site layout (device entry points below): the n_sites sites, in
 * site order, live in blocks of 2^block_shift consecutive sites (2 <= shift
 * <= 24; the last block may be partial), block b at dev_blocks[b] -- a DEVICE
 * array of device pointers, 16-byte aligned (hipMalloc's are), owned by the
 * caller.  Sites that arrive one file at a time need not be copied into one
 * allocation, and a job's 38 GB of sites and outputs spread over many
 * allocations: the fused pass's speed depended on which 38 GB buffer held its
 * output (12.8-15.2 ms on one box; blocks of 4-64 sites allocated in- and
 * output alternately ran 13.1 on every draw).  Results are
 * identical to the contiguous entry points.  Needs height*width % 8 == 0. */
int tmh_stats_update_welford_blocks_device(tmh_stats* h, const uint16_t* const* dev_blocks,
                                           int block_shift, int64_t n_sites, int log_transform,
                                           void* stream);

/* Host copies of the results; any output may be NULL.
 *   n            sites accumulated (stats.py:89)
 *   mean, std    [height*width] f64; std is NaN where n < 2 (stats.py:94-112)
 *   pct_sum      [n_quantiles] f64 running sum of per-site percentiles in
 *                site order (stats.py:76); values = int(pct_sum / n)
 *   hist         [65536] u64 pooled per-site histogram (sum over sites) */
int tmh_stats_finalize(tmh_stats* h, int64_t* n, double* mean, double* std, double* pct_sum,
                       uint64_t* hist);
/* Device form: writes mean/std planes into caller device buffers. */
int tmh_stats_finalize_device(tmh_stats* h, double* dev_mean, double* dev_std, void* stream);
/* var = M2 / (n - 1), NaN everywhere when n < 2 (stats.py:94-102), host copy. */
int tmh_stats_variance(tmh_stats* h, double* host_var);
/* Pixel groups (8 consecutive pixels of one site) holding a value >= 4,096
 * in the sites passed to tmh_stats_update_welford_device since the last fused
 * pass consumed them (synchronous; diagnostics: the automatic fused
 * configuration compares it with 2% of the groups).  sites_out may be NULL. */
int tmh_stats_wide_groups(tmh_stats* h, uint64_t* groups_out, int64_t* sites_out);
/* The current job's site probe and the automatic choices it made (see the
 * options above): probe_counts[3] = groups sampled, groups with a value >=
 * 4,096, >= 16,384 (zeros before the probe ran); welford_bright = 1 / 0, -1
 * if the job has not been probed; fused_cfg = the configuration the fused
 * pass runs (3, 5 or TMH_FUSED_NO_HIST).  Any output may be NULL. */
#define TMH_FUSED_NO_HIST 100
int tmh_stats_job_choice(tmh_stats* h, uint32_t* probe_counts, int* welford_bright,
                         int* fused_cfg);
/* Per-site histogram of the most recent update batch (debug/parity). */
int tmh_stats_site_histogram(tmh_stats* h, int64_t site_in_last_batch, uint32_t* host_hist);
/* Order statistics at every quantile's previous/next sorted position for one
 * site (last batch; any stored site in deferred mode) — debug/parity. */
int tmh_stats_site_order_stats(tmh_stats* h, int64_t site, uint16_t* host_vlo,
                               uint16_t* host_vhi);

/* ---- multi-GPU merge (one process per GPU; collectives done by the caller
 * over RCCL on the device buffers these functions fill/consume).  Every
 * entry point below that takes a stream follows the updates' stream
 * contract: on another stream than the handle's it runs after the handle's
 * queued work and the handle's stream waits for it (so one stream can merge
 * several handles -- a rank's channels -- with batched collectives). ---- */
int tmh_stats_get_n(tmh_stats* h, int64_t* n);
/* The reference's plain attribute OnlineStatistics.n (stats.py:53): the count
 * later Welford updates continue from and percentiles / var divide by. */
int tmh_stats_set_n(tmh_stats* h, int64_t n);
/* dev_nmean = n_r * mean_r (input of all_reduce(sum)) */
int tmh_stats_merge_stage1(tmh_stats* h, double* dev_nmean, void* stream);
/* mean = dev_sum_nmean / n_total; dev_m2c = M2_r + n_r * (mean_r - mean)^2 */
int tmh_stats_merge_stage2(tmh_stats* h, const double* dev_sum_nmean, int64_t n_total,
                           double* dev_m2c, void* stream);
/* Adopt the merged state: n = n_total, mean from stage 2, M2 = dev_sum_m2c. */
int tmh_stats_merge_stage3(tmh_stats* h, int64_t n_total, const double* dev_sum_m2c,
                           void* stream);
/* Percentile chain: dev_acc[n_quantiles] += each local site's percentiles,
 * in local site order (deferred mode).  Rank r runs this on the accumulator
 * received from rank r-1, keeping the reference's sequential summation. */
int tmh_stats_pct_accumulate(tmh_stats* h, double* dev_acc, void* stream);
/* Same for quantiles [q_begin, q_begin + q_count) only; dev_acc_range points at
 * the range's first element.  Lets the rank chain run as a pipeline over
 * quantile chunks (rank r adds chunk c while rank r-1 adds chunk c+1); each
 * quantile still sees every rank's sites in order (bit-exact). */
int tmh_stats_pct_accumulate_range(tmh_stats* h, double* dev_acc_range, int q_begin, int q_count,
                                   void* stream);
int tmh_stats_set_pct_sum(tmh_stats* h, const double* dev_acc, void* stream);
/* Device copy of the percentile sums (what tmh_stats_finalize's pct_sum
 * returns; deferred mode: summed in site order first unless a chain result
 * was installed), ordered on `stream` -- lets a pipelined caller keep a job's
 * results before the handle is reused, without a host synchronisation. */
int tmh_stats_get_pct_sum_device(tmh_stats* h, double* dev_acc, void* stream);
/* Pooled 65,536-bin u64 histogram out of / into the handle (device buffers):
 * the histogram merge is get -> all_reduce(sum) -> set.  Sums of counts are
 * exact, so any reduction order gives the same bins. */
int tmh_stats_get_hist_device(tmh_stats* h, uint64_t* dev_hist, void* stream);
int tmh_stats_set_hist_device(tmh_stats* h, const uint64_t* dev_hist, void* stream);

/* ---- smoothing -----------------------------------------------------------
 * Replaces tmlib/image.py:287-311 Image.smooth -> mahotas.gaussian_filter
 * (image.py:303) as used by IllumstatsContainer.smooth (image.py:1172-1193):
 * separable Gaussian, radius int(4*sigma+0.5), normalised taps, 'reflect'
 * border, float64, axis 0 then axis 1.  in == out is allowed. */
int tmh_smooth_f64(const double* host_in, double* host_out, int height, int width, double sigma);
int tmh_smooth_f64_device(const double* dev_in, double* dev_out, double* dev_tmp, int height,
                          int width, double sigma, void* stream);
/* The same for two planes (a job's mean and std, image.py:1185-1186) in one
 * launch per axis; bit-identical to two tmh_smooth_f64_device calls.
 * dev_tmp0 / dev_tmp1: scratch planes of their own. */
int tmh_smooth2_f64_device(const double* dev_in0, const double* dev_in1, double* dev_out0,
                           double* dev_out1, double* dev_tmp0, double* dev_tmp1, int height,
                           int width, double sigma, void* stream);

/* ---- correction ------------------------------------------------------------
 * Replaces tmlib/image.py:599-631 ChannelImage._correct_illumination,
 * image.py:633-670 correct, and image.py:570-597 clip.
 * A corrector holds the per-pixel affine form of the correction for one
 * (mean, std) pair:  log: out = 10**(a*log10(x) + b), a = mean(std)/std,
 * b = mean(mean) - mean*a, x==0 -> log10(1e-10);  no log: out = a*x + b.
 * lut_zero_log10 = np.log10(1e-10) from the host numpy.  The float result is
 * cast with the x86 astype rule (trunc to int32, low bits) and optionally
 * clipped to [clip_lo, clip_hi] (clip_lo < 0: no clip). */
/* One site's alignment window (Image.align, tmlib/image.py:345-454): output
 * pixel (r, c) with 0 <= r - dst_r0 < rows and 0 <= c - dst_c0 < cols takes
 * input pixel (r - dst_r0 + src_r0, c - dst_c0 + src_c0); every other output
 * pixel is 0.  The host evaluates the reference's numpy slicing into it. */
typedef struct tmh_window {
  int32_t src_r0, src_c0, dst_r0, dst_c0, rows, cols;
} tmh_window;

typedef struct tmh_corrector tmh_corrector;

int tmh_corrector_create(const double* host_mean, const double* host_std, int height, int width,
                         int log_transform, double zero_log10, tmh_corrector** out);
int tmh_corrector_create_device(const double* dev_mean, const double* dev_std, int height,
                                int width, int log_transform, double zero_log10, void* stream,
                                tmh_corrector** out);
void tmh_corrector_destroy(tmh_corrector* c);
/* Recompute the coefficients in place from new device planes (no allocation,
 * no synchronisation): one corrector serves every job of the same shape. */
int tmh_corrector_update_device(tmh_corrector* c, const double* dev_mean, const double* dev_std,
                                void* stream);
/* Options of a corrector: TMH_OPT_COPY_THREADS (see tmh_stats_set_option), and TMH_OPT_FUSED_CUS: the fused correct+histogram
 * pass's persistent grid spans this many CUs' worth of workgroups (0 or the
 * CU count, default: all) -- fewer leave room for other streams' kernels
 * (several channel jobs sharing a GPU).  Results never depend on them. */
#define TMH_OPT_FUSED_CUS 8
/* TMH_OPT_FUSED_BANDS: pixel bands of the fused pass's unit sweep, 0
 * (default: the configuration's, doubled up to 64 while a launch has fewer
 * than 8 units per workgroup -- short launches, e.g. a rank's 432-site share
 * of a channel at N = 8), or 8 / 16 / 32 / 64. */
#define TMH_OPT_FUSED_BANDS 9
int tmh_corrector_set_option(tmh_corrector* c, int option, int value);
/* The two global means (np.mean(std), np.mean(mean), image.py:627). */
int tmh_corrector_means(tmh_corrector* c, double* mean_of_std, double* mean_of_mean);
/* tmh_corrector_update_device for n <= 8 correctors (a rank's channels) in
 * one launch per kernel (the plane sums, every coefficient form, the launch
 * constants), on `stream` (NULL: the first corrector's); results identical
 * to n separate calls. */
int tmh_corrector_update_multi_device(tmh_corrector* const* cs, int n, const double* const* dev_mean,
                                      const double* const* dev_std, void* stream);
/* The planes step of n <= 8 jobs at once (a rank's channels, configs[2]/[3];
 * reference: one corilla job per channel, tmlib/workflow/corilla/api.py:64-105):
 * per job k, statistics finalize (stats.py:94-112) -> IllumstatsContainer
 * smoothing of mean and std (image.py:1172-1193, sigma) -> corrector k's
 * coefficients from the smoothed planes (image.py:599-631).  One launch per
 * kernel for all jobs: the smoothing reads each handle's mean and M2 and
 * finalizes std as it reads it (sigma 5; other sigmas finalize into scratch
 * first), then the coefficient launches of tmh_corrector_update_multi_device.
 * dev_smean / dev_sstd [n]: the smoothed planes (device, f64 [height*width]);
 * dev_mean / dev_std (may be NULL, or hold NULL entries): the unsmoothed
 * planes, written only where asked for.  Runs on `stream` (NULL: the first
 * handle's) after everything queued on every handle's stream, and every
 * handle's stream waits for it.  Results identical to finalize + smooth2 +
 * corrector update per job. */
int tmh_job_planes_multi_device(tmh_stats* const* hs, tmh_corrector* const* cs, int n,
                                double* const* dev_mean, double* const* dev_std,
                                double* const* dev_smean, double* const* dev_sstd, double sigma,
                                void* stream);
/* Host buffers: chunks of <= 16 sites, H2D / kernel / D2H on three streams
 * with two device and two pinned output slots.  Returns when host_out is
 * complete; host_out must not overlap host_in. */
int tmh_correct_u16(tmh_corrector* c, const uint16_t* host_in, uint16_t* host_out,
                    int64_t n_sites, int clip_lo, int clip_hi);
/* Device buffers, queued on `stream` (NULL: the corrector's).  dev_in and
 * dev_out must not overlap: the f64 refinement re-reads the input pixels it
 * redoes after the streaming kernel has stored the output, so an in-place
 * call would correct those pixels twice.  Overlapping ranges are rejected
 * with TMH_EINVAL, nothing launched. */
int tmh_correct_u16_device(tmh_corrector* c, const uint16_t* dev_in, uint16_t* dev_out,
                           int64_t n_sites, int clip_lo, int clip_hi, void* stream);
/* Correct n_sites pending sites of h and fold their histograms/percentiles
 * into h (see tmh_stats_update_welford_device).  Stream contract: the work
 * runs on `stream` (NULL: the corrector's stream), ordered after everything
 * already queued on h's stream, and h's stream waits for it before any later
 * work on h -- the two handles may live on different streams.  On another
 * stream than h's, the histogram tail (per-site order statistics, percentile
 * sums) runs on a stream of h's own, which h's stream waits for:
 * `stream` is free once the corrected sites are written, so a caller can
 * start its next job under this one's tail.
 * dev_in and
 * dev_out must not overlap (the pass re-reads its input after storing
 * outputs: f64 fixups, packed-counter recounts; overlapping runs are
 * rejected with TMH_EINVAL, and the block entry point's tables must name
 * separate blocks). */
int tmh_correct_u16_hist_device(tmh_corrector* c, tmh_stats* h, const uint16_t* dev_in,
                                uint16_t* dev_out, int64_t n_sites, int clip_lo, int clip_hi,
                                void* stream);
/* The same on the blocked layout (see tmh_stats_update_welford_blocks_device):
 * input and output block tables with the same block_shift; the correction's
 * zero_log10 must lie in [-37, 0] (the fused pass). */
int tmh_correct_u16_hist_blocks_device(tmh_corrector* c, tmh_stats* h,
                                       const uint16_t* const* dev_in_blocks,
                                       uint16_t* const* dev_out_blocks, int block_shift,
                                       int64_t n_sites, int clip_lo, int clip_hi, void* stream);
/* n <= 8 jobs' tmh_correct_u16_hist_device (the same image size and
 * transform, each job its own corrector and statistics handle, n_sites[k]
 * pending sites of handle k) in ONE fused launch when their configurations
 * agree (a rank's channels: a short job's launch otherwise pays the pass's
 * fill and drain on its own); a job whose configuration differs, or which
 * needs the two-pass path, gets its own launch on the same stream.  Runs on
 * `stream` (NULL: the first corrector's); the stream contract of the
 * single-job call holds for every job (each after its handle's queued work,
 * each handle's stream after its job's tail).  Results identical to the
 * per-job calls. */
int tmh_correct_u16_hist_multi_device(tmh_corrector* const* cs, tmh_stats* const* hs, int n,
                                      const uint16_t* const* dev_in, uint16_t* const* dev_out,
                                      const int64_t* n_sites, int clip_lo, int clip_hi,
                                      void* stream);
/* The same on the blocked layout: per job an input and an output block table
 * (device arrays of block pointers), one block_shift for all. */
int tmh_correct_u16_hist_multi_blocks_device(tmh_corrector* const* cs, tmh_stats* const* hs,
                                             int n, const uint16_t* const* const* dev_in_blocks,
                                             uint16_t* const* const* dev_out_blocks,
                                             int block_shift, const int64_t* n_sites, int clip_lo,
                                             int clip_hi, void* stream);
int tmh_correct_u8(tmh_corrector* c, const uint8_t* host_in, uint8_t* host_out, int64_t n_sites,
                   int clip_lo, int clip_hi);
/* ---- illuminati chain ------------------------------
 * Image.align (tmlib/image.py:412-454) of n_sites images [n][height][width] of
 * elem_bytes 1 (uint8) or 2 (uint16) into [n][out_height][out_width]: crop=True
 * gives out = window extent, crop=False out = input size, zero padded. */
int tmh_align(const void* host_in, void* host_out, int elem_bytes, int64_t n_sites, int height,
              int width, const tmh_window* windows, int out_height, int out_width);
/* ChannelImage._map_to_uint8 (tmlib/image.py:493-531) with explicit bounds
 * (0 <= lower < upper <= 65535): the reference's numpy LUT, bit-exact. */
int tmh_map_u16_to_u8(const uint16_t* host_in, uint8_t* host_out, int64_t n, int lower,
                      int upper);
/* illuminati/api.py:396-405 in one pass: correct (this corrector's statistics)
 * -> align(crop=False) with each site's window -> clip(clip_lo, clip_hi) ->
 * scale(clip_lo, clip_hi) to uint8.  Corrected values within +-1 DN of the
 * reference before the clip/scale (the +-1 DN bar of the correction). */
int tmh_correct_chain_u8_device(tmh_corrector* c, const uint16_t* dev_in, uint8_t* dev_out,
                                int64_t n_sites, const tmh_window* host_windows, int clip_lo,
                                int clip_hi, void* stream);
int tmh_correct_chain_u8(tmh_corrector* c, const uint16_t* host_in, uint8_t* host_out,
                         int64_t n_sites, const tmh_window* host_windows, int clip_lo,
                         int clip_hi);

/* ---- illuminati tile pyramid ------------------------------------------------
 * Replaces the pixel work of tmlib/workflow/illuminati/api.py:356-501
 * (_create_maxzoom_level_tiles: every site stitched into 256 x 256 base tiles,
 * with pixels of the upper and left neighbours) and :503-573
 * (_create_lower_zoom_level_tiles: 2 x 2 tile mosaic -> Image.shrink).
 * Tile-major storage: a level is [tile_rows][tile_cols][256][256] uint8, each
 * tile 64 KB contiguous; a ragged tile (last row / column of a level) lies in
 * its tile's top left corner at the 256-byte row pitch, zeros around it.
 *
 * One rectangle of the base gather: tile `tile` (row-major index) takes
 * height x width bytes of site `site` from (src_y, src_x) at (dst_y, dst_x).
 * The host evaluates the reference's extract / pad / insert rules into the
 * table (tmlibrary_amd/workflow/pyramid.py); rectangles of one tile must be
 * disjoint (which of two overlapping ones a byte takes is unspecified). */
typedef struct tmh_tile_rect {
  int32_t tile, site, src_y, src_x, dst_y, dst_x, height, width;
} tmh_tile_rect;
/* Gather host_rects[n_rects] (any order) from dev_sites [n_sites][height][width]
 * uint8 (tmh_correct_chain_u8_device's output) into dev_tiles
 * [tile_rows][tile_cols][256][256]: every byte of every tile is written once,
 * 0 where no rectangle covers it (spacer tiles are all 0: what api.py:550
 * substitutes for a missing base tile).  dev_tiles 16-byte aligned.  The
 * table is checked first (a rectangle leaving its site or tile, an index out
 * of range, a non-positive size: TMH_EINVAL, nothing launched), then uploaded
 * and the gather queued on `stream` (NULL: the default stream); the call
 * returns once the gather has run (it frees the uploaded table), so
 * host_rects may be reused at once. */
int tmh_tiles_base_device(const uint8_t* dev_sites, int64_t n_sites, int height, int width,
                          const tmh_tile_rect* host_rects, int64_t n_rects, uint8_t* dev_tiles,
                          int tile_rows, int tile_cols, void* stream);
int tmh_tiles_base(const uint8_t* host_sites, int64_t n_sites, int height, int width,
                   const tmh_tile_rect* host_rects, int64_t n_rects, uint8_t* host_tiles,
                   int tile_rows, int tile_cols);
/* One level to the next: output tile (y, x) of the ceil(src_rows / 2) x
 * ceil(src_cols / 2) output level is the mosaic of source tiles (2y..2y+1,
 * 2x..2x+1) that exist, halved with (a + b + c + d + 2) >> 2 per pixel
 * (OpenCV's integer INTER_AREA path at scale 2 on uint8, which Image.shrink,
 * image.py:313-343, reaches through cv2.resize).  Only the last tile row /
 * column of a level may be smaller than 256: src_last_h / src_last_w (1..256)
 * give theirs, *dst_last_h / *dst_last_w report the output level's (half the
 * last mosaic's side, rounded down; TMH_EINVAL if that is 0).  A mosaic with
 * an odd side has no scale-2 path: its output tile is NOT written (the caller
 * computes it, pyramid.py's exact area mean); every other output tile is
 * written whole, zeros outside its ragged extent.  Both levels 16-byte
 * aligned and distinct.  Asynchronous on `stream` (NULL: the default
 * stream); the host form is synchronous and keeps host_dst's bytes in the
 * tiles it does not write. */
int tmh_pyramid_shrink2_device(const uint8_t* dev_src, int src_rows, int src_cols, int src_last_h,
                               int src_last_w, uint8_t* dev_dst, int* dst_last_h, int* dst_last_w,
                               void* stream);
int tmh_pyramid_shrink2(const uint8_t* host_src, int src_rows, int src_cols, int src_last_h,
                        int src_last_w, uint8_t* host_dst, int* dst_last_h, int* dst_last_w);
/* JPEG-code every tile of one tile-major level: what PyramidTile.jpeg_encode
 * (image.py:1073-1094, cv2.imencode('.jpeg', array, [IMWRITE_JPEG_QUALITY,
 * quality])) returns for each tile and ChannelLayerTile.pixels stores
 * (models/tile.py:107-122), for all rows x cols tiles in one call.  The first
 * five arguments are a level as the calls above leave it: tile (y, x) is
 * last_h high in the last row, last_w wide in the last column (1..256), 256
 * otherwise, and only that extent is the image -- the bytes around a ragged
 * tile are not read as samples.  Every file is the baseline JPEG libjpeg
 * writes for one 8-bit grayscale component, byte for byte: SOI, APP0 JFIF
 * 1.01 (no units, density 1 x 1), DQT (table 0 of jpeg_set_quality(quality,
 * force_baseline), quality clamped to 1..100), SOF0 with the tile's height
 * and width, the Annex K.3 / K.5 luminance Huffman tables, SOS, the
 * entropy-coded segment and EOI -- a 328-byte header; blocks padded by
 * replicating the last column, then the last row; jfdctint.c's slow-integer
 * DCT; one DC predictor per tile, no restart markers; 0xFF bytes stuffed, the
 * last byte filled with 1 bits.
 * dev_offsets[rows * cols + 1] is always filled: offsets[0] = 0, then the
 * exclusive scan of the exact file sizes in row-major tile order; *total
 * (host) = offsets[rows * cols].  dev_out NULL: the call only measures.
 * Otherwise tile t's file is written at dev_out + offsets[t] (one compact
 * blob; no byte past *total is touched); out_capacity < *total: TMH_EINVAL
 * with *total set and nothing written to dev_out.  A NULL level, offsets or
 * total, rows or cols < 1, last_h or last_w outside 1..256: TMH_EINVAL,
 * nothing launched.  dev_level 16-byte, dev_offsets 8-byte aligned.  A level
 * is coded once to measure and, when writing, once more at the offsets; work
 * is queued on `stream` (NULL: the default stream) and the call returns when
 * the result is complete. */
int tmh_jpeg_encode_level_device(const uint8_t* dev_level, int rows, int cols, int last_h,
                                 int last_w, int quality, uint8_t* dev_out, int64_t out_capacity,
                                 int64_t* dev_offsets, int64_t* total, void* stream);
int tmh_jpeg_encode_level(const uint8_t* host_level, int rows, int cols, int last_h, int last_w,
                          int quality, uint8_t* host_out, int64_t out_capacity,
                          int64_t* host_offsets, int64_t* total);
/* Every tile of a level as libjpeg decodes it from the file
 * tmh_jpeg_encode_level writes for it at `quality`: what the getter
 * ChannelLayerTile.pixels (models/tile.py:97-105, PyramidTile.create_from_binary,
 * cv2.imdecode) hands to _create_lower_zoom_level_tiles (illuminati/api.py:
 * 503-573) when it reads the level above.  No file is made: Huffman coding is
 * lossless, so per 8 x 8 block (padded by replicating the last column, then the
 * last row) it is the encoder's forward DCT and quantiser, then coefficient x
 * the file's 8-bit quantiser, jidctint.c's slow-integer inverse DCT
 * (jpeg_idct_islow: columns first with DESCALE by 11, then rows with DESCALE by
 * 18) and the range limit clamp(v + 128, 0, 255), cropped to the tile's
 * extent.  The first five arguments are a level as for the encoder; dev_out
 * has the same layout and every byte of it is written once: the decoded
 * samples inside a tile's extent, 0 around a ragged tile.  A NULL pointer, rows
 * or cols < 1, last_h or last_w outside 1..256, dev_out == dev_level (the
 * levels must not overlap): TMH_EINVAL, nothing launched.  Both 16-byte
 * aligned.  Asynchronous on `stream` (NULL: the default stream); the host form
 * is synchronous. */
int tmh_jpeg_roundtrip_level_device(const uint8_t* dev_level, int rows, int cols, int last_h,
                                    int last_w, int quality, uint8_t* dev_out, void* stream);
int tmh_jpeg_roundtrip_level(const uint8_t* host_level, int rows, int cols, int last_h, int last_w,
                             int quality, uint8_t* host_out);
/* Decode n stored tile files (PyramidTile.create_from_binary, image.py:993-1037)
 * in one call.  File t is dev_blob[offsets[t] .. offsets[t + 1]) (offsets: n + 1
 * entries, not decreasing; an EncodedLevel's blob and offsets fit as they are).
 * Tile t is written to dev_tiles + t * 65536 in the level storage's form: the
 * picture at a 256-byte pitch in the corner, 0 around it; dims[2 t], dims[2 t
 * + 1] = its height and width; status[t] = 0.  A file that is not decoded
 * leaves a tile of zeros, dims (0, 0) and status 1 (well formed but not
 * supported) or 2 (corrupt); the call still returns TMH_OK.
 * Decoded: every file libjpeg writes for one 8-bit grayscale component with
 * default settings at any quality -- SOI; APPn, COM and unknown segments
 * passed over; DQT 8-bit, table 0, values 1..255 (other table ids ignored);
 * SOF0 with precision 8, one component sampled 1 x 1 using table 0, height and
 * width in 1..256; DHT class 0 and 1, id 0, equal to Annex K.3 / K.5, one or
 * several tables to a segment; DRI with interval 0; SOS with Ss 0, Se 63, Ah
 * = Al = 0; one DC predictor, 0xFF 0x00 unstuffed; EOI directly after the last
 * block's padded byte (bytes after EOI are ignored).  The pixels are
 * libjpeg's: tmh_jpeg_roundtrip_level's arithmetic.
 * Status 1: SOF1, SOF2 and above, DNL or arithmetic conditioning; precision
 * other than 8; more than one component; other sampling or table selectors;
 * a side of 0 or above 256; a 16-bit or missing table 0 DQT; missing or
 * non-Annex-K Huffman tables; a non-zero restart interval; a scan that is not
 * 0..63 / 0.  Status 2: no SOI; a header or segment that does not fit the file
 * or is malformed; a zero quantiser; the coded data ending (or a marker
 * standing) before the last block is complete; a bit pattern that is no code;
 * a run past coefficient 63; a DC category above 11, an AC size above 10 or a
 * DC value outside -2048..2047; anything but EOI after the last block.
 * For any bytes no read leaves a file's range and no write its tile's 64 KB.
 * n < 0, a NULL pointer (n > 0; offsets always) or, in the host form,
 * decreasing or negative offsets: TMH_EINVAL, nothing launched.  n = 0 does
 * nothing.  dev_tiles 16-byte, dev_offsets 8-byte, dims and status 4-byte
 * aligned.  Queued on `stream` (NULL: the default stream); the call returns
 * when the result is complete. */
int tmh_jpeg_decode_tiles_device(const uint8_t* dev_blob, const int64_t* dev_offsets, int64_t n,
                                 uint8_t* dev_tiles, int32_t* dev_dims, int32_t* dev_status,
                                 void* stream);
int tmh_jpeg_decode_tiles(const uint8_t* host_blob, const int64_t* host_offsets, int64_t n,
                          uint8_t* host_tiles, int32_t* host_dims, int32_t* host_status);

/* ---- registration: the align step's shifts ---------------------------------
 * Replaces tmlib/workflow/align/registration.py:23-86 (calculate_shift, i.e.
 * image_registration.chi2_shift rounded to integers) for every (target,
 * reference) pair of a job (tmlib/workflow/align/api.py:157-260).
 *
 * For a target T and a reference R of the same shape H x W, from the
 * mean-removed images (exact integer sums),
 *     C[dy, dx] = sum_{r,c} T[r, c] * R[(r + dy) mod H, (c + dx) mod W]
 * and the shift is the argmax of C in signed form: a lag d along an axis of
 * length L is d when d <= L / 2 (integer division), else d - L.  So (y, x)
 * means T[r, c] ~ R[r + y, c + x], the sign _shift_and_crop expects.  Ties go
 * to the lowest flat unsigned lag dy * W + dx; a pair in which either image is
 * constant has C = 0 exactly and gives (0, 0) with peak 0.
 * C is computed in f32 by a 2-D FFT; an axis whose length has a prime factor
 * above 5 is zero-padded to a 5-smooth length >= 2 L - 1 and the linear
 * correlation folded back to period L.  A transformed line holds at most 4,096
 * values: an axis is at most 4,096 when 5-smooth and at most 2,048 otherwise
 * (TMH_EINVAL beyond).
 *
 * targets [n][H][W] and references [m][H][W] of elem_bytes 1 (uint8) or 2
 * (uint16); target i is registered against reference ref_of_target[i] (host,
 * each in 0..m-1).  y, x (host, n) and peak (host, n, may be NULL: C at the
 * argmax) are filled when the call returns.  dev_scratch: at least
 * tmh_register_scratch_bytes(n, m, H, W) bytes, 256-byte aligned (that
 * function returns a negative code for arguments the calls reject).  Queued on
 * `stream` (NULL: the default stream).  n = 0 does nothing. */
int64_t tmh_register_scratch_bytes(int64_t n, int64_t m, int height, int width);
int tmh_register_shifts_device(const void* dev_targets, int64_t n, const void* dev_refs, int64_t m,
                               int height, int width, int elem_bytes,
                               const int32_t* host_ref_of_target, void* dev_scratch,
                               int64_t scratch_bytes, int32_t* host_y, int32_t* host_x,
                               float* host_peak, void* stream);
int tmh_register_shifts(const void* host_targets, int64_t n, const void* host_refs, int64_t m,
                        int height, int width, int elem_bytes, const int32_t* ref_of_target,
                        int32_t* y, int32_t* x, float* peak);
/* The f32 plane C[H][W] of one pair, in unsigned lag order (scratch as for
 * n = m = 1).  The device form returns when the plane is complete. */
int tmh_xcorr_plane_device(const void* dev_target, const void* dev_ref, int height, int width,
                           int elem_bytes, void* dev_scratch, int64_t scratch_bytes,
                           float* dev_plane, void* stream);
int tmh_xcorr_plane(const void* host_target, const void* host_ref, int height, int width,
                    int elem_bytes, float* host_plane);

/* ChannelImage.clip alone (image.py:589), u16. */
int tmh_clip_u16(const uint16_t* host_in, uint16_t* host_out, int64_t n, int lo, int hi);

/* ---- synthetic input (imextract stand-in for benchmarks) -----------------
 * Sites [first_site, first_site + n_sites) of (seed, channel), generated in
 * HBM with integer arithmetic only, so tmlibrary_amd/synth.py
 * (synth_exact_host) reproduces every pixel bit for bit on the host and the
 * bench's full-size results can be checked against the CPU oracle.
 * distribution: TMH_SYNTH_STANDARD  100 + vignetting * LogNormal(6, 0.6) + N(0, 5)
 *               TMH_SYNTH_BRIGHT    the same with LogNormal(8.5, 0.6) (median ~5,000)
 *               TMH_SYNTH_UNIFORM   uniform 0..65535
 * (STANDARD / BRIGHT also carry 0.01 % zeros and 0.01 % saturated pixels.) */
#define TMH_SYNTH_STANDARD 0
#define TMH_SYNTH_BRIGHT 1
#define TMH_SYNTH_UNIFORM 2
int tmh_synth_sites_device(uint16_t* dev_out, int64_t n_sites, int height, int width,
                           uint64_t seed, int channel, int64_t first_site, int distribution,
                           void* stream);
/* The generator's integer tables (host only, no GPU needed): ln16/nz16
 * [4096] (lognormal and noise quantiles in 1/16 DN), ey[height], ex[width]
 * (vignetting factors, 2^15 = 1). */
int tmh_synth_tables(int distribution, int height, int width, int32_t* ln16, int32_t* nz16,
                     int32_t* ey, int32_t* ex);

/* ---- box probe (bench support; no reference counterpart) ------------------
 * The box's own stream rates for the two passes' bytes, so a bench line can
 * tell a slow box from a slow kernel: even modes copy -- read every site's 2
 * B/px and write them to its output block (the fused correct+histogram pass's
 * bytes) --, odd modes read every site once (the Welford pass's); 16-byte
 * non-temporal loads and stores as the passes move them, over the caller's
 * blocked layout (device block tables as in
 * tmh_stats_update_welford_blocks_device; shift 24 with one entry: one
 * contiguous run; dev_out_blocks unused when reading).  Modes 0 / 1: one
 * persistent grid-strided launch; 2 / 3: one thread per 16 bytes, one launch
 * per block.  reps repetitions on `stream`; ms_out = their average (HIP
 * events), sclk_mhz_out (may be NULL) = the shader clock during the last
 * persistent launch (clock64 ticks per 100 MHz wall_clock64 tick in
 * workgroup 0; 0 for modes 2 / 3).  Synchronous.  The copy modes overwrite
 * the output blocks with the sites: probe before the outputs are produced or
 * after they have been checked. */
int tmh_box_probe_device(const uint16_t* const* dev_in_blocks, uint16_t* const* dev_out_blocks,
                         int block_shift, int64_t n_sites, int height, int width, int mode,
                         int reps, void* stream, double* ms_out, double* sclk_mhz_out);

/* ---- site-image input: GPU inflate of HDF5 gzip chunks ------------------
 * Replaces the deflate filter libhdf5 runs under h5py for every chunk of a
 * ChannelImageFile's /array (tmlib/models/file.py:322-351,
 * tmlib/readers.py:367-389; written by file.py:353-363, writers.py:384-387):
 * each chunk is an independent zlib stream (RFC 1950/1951), decoded by one
 * GPU lane.  The compressed chunks of many files (libtmh5's
 * tmh5_read_raw_chunks fills the same table layout) sit in one device
 * buffer; tmh_inflate_device writes chunk i's raw_len decompressed bytes at
 * dev_raw + raw_off and its status (TMH_Z_*; 0 = ok) -- byte-identical to
 * zlib's inflate, Adler-32 checked.  tmh_place_chunks_device then copies
 * every chunk's rows into dev_images[image][height][width] (elem_bytes per
 * element), clipping edge chunks to the dataset's extent. */
#define TMH_ZCHUNK_STORED 1 /* the deflate filter was skipped: raw bytes stored */
typedef struct tmh_zchunk {
  int64_t src_off;    /* the chunk's zlib stream in the compressed buffer */
  int64_t src_len;
  int64_t raw_off;    /* its decompressed bytes in the raw buffer */
  int64_t raw_len;    /* chunk_rows * chunk_cols * elem_bytes */
  int64_t image;      /* destination image of tmh_place_chunks_device */
  int32_t row0, col0; /* chunk origin in the image, elements */
  int32_t flags;      /* TMH_ZCHUNK_STORED */
  int32_t reserved;
} tmh_zchunk;
#define TMH_Z_OK 0
#define TMH_Z_HEADER 1     /* not a zlib stream (CM/CINFO/FCHECK/FDICT) */
#define TMH_Z_BLOCKTYPE 2  /* deflate block type 3 */
#define TMH_Z_CODE 3       /* a code the block's Huffman tables do not hold */
#define TMH_Z_DIST 4       /* a back-reference before the start of the chunk */
#define TMH_Z_OVERFLOW 5   /* more than raw_len bytes */
#define TMH_Z_INPUT 6      /* ran past the chunk's bytes / bad offsets */
#define TMH_Z_ADLER 7      /* Adler-32 mismatch */
#define TMH_Z_SIZE 8       /* fewer than raw_len bytes */
#define TMH_Z_STORED 9     /* stored block LEN / NLEN mismatch */
/* TMH_Z_TABLE also covers the incomplete codes zlib's inflate_table rejects:
 * a code that leaves bit patterns unused is taken only as exactly one code of
 * length 1 (for distances also as no code at all), never for the code-length
 * code. */
#define TMH_Z_TABLE 10     /* invalid code lengths (over-subscribed, incomplete, no end code) */
/* Two kernels: each lane Huffman-decodes one chunk, writing its literal bytes
 * and listing its back-references in dev_scratch (no lane waits on a load of
 * earlier output); then one wave per chunk resolves the list in order, 64
 * matches at a time, and checks the Adler-32.  raw_max: the largest raw_len
 * of the table; dev_scratch: at least tmh_inflate_scratch_bytes(n_chunks,
 * raw_max) bytes, 16-byte aligned.  TMH_INFLATE_LANES (4..64, env) sets the
 * streams per phase-1 workgroup (default: from n_chunks and the CU count). */
int64_t tmh_inflate_scratch_bytes(int64_t n_chunks, int64_t raw_max);
int tmh_inflate_device(const uint8_t* dev_src, int64_t src_bytes, const tmh_zchunk* dev_chunks,
                       int64_t n_chunks, int64_t raw_max, uint8_t* dev_raw, int64_t raw_bytes,
                       void* dev_scratch, int64_t scratch_bytes, int32_t* dev_status,
                       void* stream);
int tmh_place_chunks_device(const uint8_t* dev_raw, const tmh_zchunk* dev_chunks, int64_t n_chunks,
                            int height, int width, int elem_bytes, int chunk_rows, int chunk_cols,
                            void* dev_images, void* stream);

/* ---- site-image output: GPU deflate of HDF5 gzip chunks -----------------
 * The mirror of the input path, for imextract
 * (tmlib/workflow/imextract/api.py:88-157: the planes of a site, their
 * elementwise maximum when there are several, ChannelImageFile.put) and any
 * caller with sites on the device.  tmh_gather_chunks_device cuts
 * dev_images[n_images][height][width] (elem_bytes 1 or 2) into chunk-major
 * raw bytes, edge chunks padded with zeros (HDF5's fill value), and fills
 * raw_off, raw_len, image, row0, col0 of the n_images * ceil(height /
 * chunk_rows) * ceil(width / chunk_cols) table entries (image-major, then
 * row-major chunks).  tmh_deflate_device codes every chunk as one complete
 * zlib stream (RFC 1950: CM 8, CINFO 7, dynamic-Huffman or stored blocks,
 * Adler-32), packs the streams into dev_dst in table order and fills src_off
 * and src_len: the table then feeds tmh_inflate_device and libtmh5's
 * tmh5_write_channel_images_raw_chunks unchanged.  No stream is longer than
 * tmh_deflate_bound(raw_len); dst_bytes must be at least n_chunks *
 * tmh_deflate_bound(raw_max).  dev_status: TMH_Z_OK, or TMH_Z_INPUT for a
 * table entry outside the raw buffer (src_len 0).  *dev_total_bytes (device
 * memory): the bytes of all streams.  dev_scratch: at least
 * tmh_deflate_scratch_bytes(n_chunks, raw_max) bytes, 16-byte aligned.  The
 * bytes depend on the input alone (tests/deflate_host.cpp builds the same
 * encoder for the CPU). */
int64_t tmh_deflate_bound(int64_t raw_len);
int64_t tmh_deflate_scratch_bytes(int64_t n_chunks, int64_t raw_max);
int tmh_gather_chunks_device(const void* dev_images, int64_t n_images, int height, int width,
                             int elem_bytes, int chunk_rows, int chunk_cols,
                             tmh_zchunk* dev_chunks, uint8_t* dev_raw, void* stream);
int tmh_deflate_device(const uint8_t* dev_raw, int64_t raw_bytes, tmh_zchunk* dev_chunks,
                       int64_t n_chunks, int64_t raw_max, uint8_t* dev_dst, int64_t dst_bytes,
                       void* dev_scratch, int64_t scratch_bytes, int32_t* dev_status,
                       int64_t* dev_total_bytes, void* stream);
/* dev_out[site] = the elementwise maximum of dev_planes[site][0..z), z >= 1
 * (np.max(np.dstack(planes), axis=2)). */
int tmh_zproject_max_device(const void* dev_planes, int64_t n_sites, int z, int height, int width,
                            int elem_bytes, void* dev_out, void* stream);
/* Host-buffer forms (unpipelined).  tmh_deflate_images: gather + deflate;
 * host_chunks and host_status hold one entry per chunk, host_blob the packed
 * streams (*total bytes; TMH_EINVAL with *total set when blob_capacity is
 * smaller). */
int tmh_deflate_images(const void* host_images, int64_t n_images, int height, int width,
                       int elem_bytes, int chunk_rows, int chunk_cols, tmh_zchunk* host_chunks,
                       uint8_t* host_blob, int64_t blob_capacity, int32_t* host_status,
                       int64_t* total);
int tmh_zproject_max(const void* host_planes, int64_t n_sites, int z, int height, int width,
                     int elem_bytes, void* host_out);

/* ---- channel images as PNG files ------------------------------------------
 * tmlib/image.py:672-682 (ChannelImage.png_encode): how a site leaves as a
 * picture.  dev_images[n_images][height][width], elem_bytes 1 or 2, become
 * n_images PNG files: greyscale (colour type 0), bit depth 8 or 16, no
 * interlace, one filter per row chosen by the smallest sum of absolute
 * filtered values, the zlib stream (CM 8, CINFO 7, as tmh_deflate_device
 * writes) cut into pieces of tmh_png_piece_bytes() filtered bytes, one IDAT
 * chunk per piece and one more for the Adler-32.  Any PNG reader decodes them
 * to the input pixels; the bytes depend on the input alone
 * (tests/png_host.cpp builds the same encoder for the CPU) but are not those
 * of libpng.  File i is dev_dst[dev_offsets[i], dev_offsets[i + 1]), the files
 * back to back; dev_offsets has n_images + 1 entries (device memory), the
 * last one the total.  No file is longer than tmh_png_bound(height, width,
 * elem_bytes); dst_bytes must be at least n_images times that.  dev_scratch:
 * at least tmh_png_scratch_bytes(...) bytes, 16-byte aligned.  Images,
 * destination, offsets and scratch must not overlap. */
int64_t tmh_png_piece_bytes(void);
int64_t tmh_png_bound(int height, int width, int elem_bytes);
int64_t tmh_png_scratch_bytes(int64_t n_images, int height, int width, int elem_bytes);
int tmh_png_encode_device(const void* dev_images, int64_t n_images, int height, int width,
                          int elem_bytes, uint8_t* dev_dst, int64_t dst_bytes,
                          int64_t* dev_offsets, void* dev_scratch, int64_t scratch_bytes,
                          void* stream);
/* Host-buffer form (unpipelined): host_offsets[n_images + 1] and the files in
 * host_blob (*total bytes; TMH_EINVAL with *total set when blob_capacity is
 * smaller). */
int tmh_png_encode(const void* host_images, int64_t n_images, int height, int width, int elem_bytes,
                   uint8_t* host_blob, int64_t blob_capacity, int64_t* host_offsets, int64_t* total);

/* ---- jterator: a site's channel stacks and object tables -------------------
 * What jterator computes around its modules (which live in another package).
 *
 * Input, tmlib/workflow/jterator/api.py:283-316 (_load_pipeline_input): every
 * plane (z-plane x time point) of a channel is corrected, aligned with
 * crop=True and written to image_array[:, :, zplane, tpoint] of a
 * (aligned_height, aligned_width, n_zplanes, n_tpoints) array.  One launch
 * for all planes of a channel: planes [n_planes][height][width] uint16, the
 * output [n_sites][out_h][out_w][slots] with slot = zplane * n_tpoints +
 * tpoint, i.e. n_sites C-ordered [out_h][out_w][n_zplanes][n_tpoints] arrays.
 * Element (site, r, c, slot) is the corrected pixel (src_r0 + r, src_c0 + c) of
 * the plane with host_site[p] == site and host_slot[p] == slot -- the value
 * tmh_correct_u16_device writes for it without a clip, bit for bit -- or the
 * raw pixel when c is NULL (a channel that is not corrected); a (site, slot)
 * no plane maps to is 0 (np.zeros), written by the same launch.  host_windows
 * [n_planes] are the planes' crop=True windows; only src_r0, src_c0, rows and
 * cols are read.  TMH_EINVAL, nothing launched: two planes on one (site,
 * slot); a window whose rows / cols differ from (out_h, out_w) (the
 * reference's numpy assignment raises there) or which leaves the source; a
 * site or slot index out of range; a corrector of another image size; more
 * than 65,535 sites; dev_out overlapping dev_in.  Both are 2-byte
 * aligned (the 16-byte forms of slots == 1 want dev_in, corrected, or
 * dev_out, not corrected, 16-byte aligned).  Queued on `stream` (NULL: the
 * corrector's, or the default stream without one); the call returns when the
 * stack is complete. */
int tmh_correct_stack_u16_device(tmh_corrector* c, const uint16_t* dev_in, uint16_t* dev_out,
                                 int64_t n_planes, int height, int width,
                                 const int32_t* host_site, const int32_t* host_slot,
                                 const tmh_window* host_windows, int64_t n_sites, int slots,
                                 int out_h, int out_w, void* stream);
int tmh_correct_stack_u16(tmh_corrector* c, const uint16_t* host_in, uint16_t* host_out,
                          int64_t n_planes, int height, int width, const int32_t* host_site,
                          const int32_t* host_slot, const tmh_window* host_windows,
                          int64_t n_sites, int slots, int out_h, int out_w);

/* Output, tmlib/workflow/jterator/handles.py:399-551 and tmlib/image.py:796:
 * the integer sums behind SegmentedObjects' labels, mh.labeled.bbox, centroids
 * (mh.center_of_mass(plane, labels=plane)) and is_border, one row per label
 * 0..max_label of one int32 label plane [height][width] (label 0, the
 * background, gets a row like any other; mahotas does the same).  Every field
 * is exact and independent of scheduling.  How a table kernel walks a label
 * plane, here and for the intensity table below: it gathers each 16 x 512
 * tile's labels in an LDS hash of TMH_OBJECT_SLOTS entries (the top 9 bits of
 * label * 2654435761 mod 2^32, linear probing); a label that finds no entry
 * within TMH_OBJECT_PROBE probes is added to its row in memory directly:
 * slower, the same result. */
#define TMH_OBJECT_SLOTS 512
#define TMH_OBJECT_PROBE 16
typedef struct tmh_object_row {
  int64_t n, sum_y, sum_x;  /* pixel count, sum of row indices, sum of column indices */
  int32_t y0, y1, x0, x1;   /* mh.labeled.bbox: [min_y, max_y+1, min_x, max_x+1]; n == 0: all 0 */
  int32_t border, pad;      /* 1 if the label occurs in row 0, row H-1, column 0 or column W-1 */
} tmh_object_row;
/* dev_max[p] / dev_min[p] = the largest / smallest label of plane p, on
 * `stream` (NULL: the default stream), asynchronously. */
int tmh_label_max_device(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                         int32_t* dev_max, int32_t* dev_min, void* stream);
/* dev_rows [n_planes][max_label + 1].  A negative label or a label above
 * max_label in any plane: TMH_EINVAL with dev_rows untouched -- found from
 * tmh_label_max_device's result, which the call computes and waits for first,
 * never by an out-of-range write.  The table is then queued on `stream`
 * (NULL: the default stream).  At most 65,535 planes per call; n_planes = 0
 * does nothing. */
int tmh_object_table_device(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                            int32_t max_label, tmh_object_row* dev_rows, void* stream);
/* Host buffers.  *max_label = the largest label of all planes (at least 0);
 * host_rows [n_planes][*max_label + 1], caller-owned like every host pointer
 * here, with room for row_capacity rows: a smaller capacity (or host_rows
 * NULL) is TMH_EINVAL with *max_label set and nothing written, so a caller
 * sizes the table from a first call.  A negative label: TMH_EINVAL. */
int tmh_object_table(const int32_t* host_planes, int64_t n_planes, int height, int width,
                     int32_t* max_label, tmh_object_row* host_rows, int64_t row_capacity);

/* SegmentationImage.extract_polygons (tmlib/image.py:778-917) up to its choice
 * of shell and holes: per label of a plane, the mask of the label inside its
 * bounding box padded by one pixel, taken from the plane with row 0, row H-1,
 * column 0 and column W-1 zeroed; mh.open (the 3x3 cross) when the mask has
 * more than one pixel; then every border cv2.findContours(RETR_CCOMP,
 * CHAIN_APPROX_NONE) follows, as Suzuki and Abe's Algorithm 1 defines them.
 * Points are (x, y) = (column, row) of the padded mask, int32 pairs; the
 * caller adds the offsets (image.py:886-893).  A box of more than
 * TMH_CONTOUR_LDS_PIXELS padded pixels is traced in memory instead of LDS:
 * slower, the same result; up to TMH_CONTOUR_LDS_SMALL_PIXELS and up to
 * TMH_CONTOUR_LDS_TINY_PIXELS it takes smaller LDS forms. */
#define TMH_CONTOUR_LDS_PIXELS 16384
#define TMH_CONTOUR_LDS_SMALL_PIXELS 4096
#define TMH_CONTOUR_LDS_TINY_PIXELS 1024
typedef struct tmh_contour {
  int32_t plane, label;
  int32_t is_hole;        /* 0: outer border, 1: hole border */
  int32_t parent;         /* a hole's outer border, as an index among the object's contours; else -1 */
  int64_t point_offset;   /* first point, as an index among all points of the call */
  int64_t n_points;
} tmh_contour;
typedef struct tmh_contour_object {
  int32_t plane, label;
  int64_t first_contour, first_point;  /* exclusive scans in (plane, label) order */
  int32_t n_contours;     /* in discovery order (raster scan); 0: the opening left nothing */
  int32_t opened;         /* the mask had more than one pixel, so mh.open ran */
  int64_t n_points;
  int64_t n_interior;     /* pixels of the label off the four border lines; 0: the label yields nothing */
  int64_t sum_y, sum_x;   /* their plane coordinates summed (image.py:835-836) */
} tmh_contour_object;
/* dev_rows: what tmh_object_table_device wrote for the same planes and
 * max_label (the planes are not read again for their label range).
 * dev_objects [n_planes][max_label + 1] is always filled; *n_contours and
 * *n_points (host) are the totals.  dev_contours and dev_points NULL: the call
 * only measures.  Otherwise object o's borders are dev_contours[first_contour
 * .. + n_contours) and its points dev_points[2 * first_point ..): one compact
 * table in (plane, label, discovery) order, identical bytes from call to call;
 * a capacity below the totals: TMH_EINVAL with the totals set and nothing
 * written to either.  Objects are traced once to measure and, when writing,
 * once more at their offsets; work is queued on `stream` (NULL: the default
 * stream) and the call returns when the result is complete. */
int tmh_object_contours_device(const int32_t* dev_planes, int64_t n_planes, int height, int width,
                               int32_t max_label, const tmh_object_row* dev_rows,
                               tmh_contour_object* dev_objects, tmh_contour* dev_contours,
                               int64_t contour_capacity, int32_t* dev_points,
                               int64_t point_capacity, int64_t* n_contours, int64_t* n_points,
                               void* stream);
/* Host buffers: the object table and the contours of host planes in one call.
 * *max_label, *n_contours and *n_points are what the planes need; host_rows
 * and host_objects hold row_capacity entries each (n_planes * (*max_label + 1)
 * needed), host_contours contour_capacity, host_points 2 * point_capacity
 * int32.  Any capacity too small (or its pointer NULL): TMH_EINVAL with the
 * three counts set and nothing written.  A negative label: TMH_EINVAL. */
int tmh_object_contours(const int32_t* host_planes, int64_t n_planes, int height, int width,
                        int32_t* max_label, tmh_object_row* host_rows,
                        tmh_contour_object* host_objects, int64_t row_capacity,
                        tmh_contour* host_contours, int64_t contour_capacity,
                        int32_t* host_points, int64_t point_capacity, int64_t* n_contours,
                        int64_t* n_points);

/* Measurement (tmlib/workflow/jterator/handles.py:840-924): the intensity
 * features of every object of a label plane, DESIGN.md section 27.  For label
 * l of a plane and one channel, the values v = I[L == l] give one integer row
 * (n == 0: all fields 0); max, mean, min, sum and std (np.std, ddof 0) follow
 * from the rows bit for bit as section 27.1 states.  Every field is
 * accumulated with integer atomics: exact, the same bytes from call to call.
 * The table kernel walks the label plane as the object table's does (above),
 * with TMH_INTENSITY_SLOTS entries and TMH_INTENSITY_PROBE probes, the same
 * numbers.  One pass holds up to TMH_INTENSITY_PASS_CHANNELS channels; more
 * channels are more passes inside the call. */
#define TMH_INTENSITY_SLOTS 512
#define TMH_INTENSITY_PROBE 16
#define TMH_INTENSITY_PASS_CHANNELS 4
#define TMH_INTENSITY_MAX_CHANNELS 16
typedef struct tmh_intensity_row {
  uint64_t sum, sum_sq;  /* of the values, of their squares */
  int64_t n;             /* pixel count */
  uint32_t min, max;
} tmh_intensity_row;
/* dev_labels [n_planes][height][width] int32; pixel (channel c, plane p, row y,
 * column x) is element c * channel_stride + p * plane_stride + y * row_stride
 * + x * pix_stride of dev_pixels, elements of elem_bytes (1: uint8, 2: uint16)
 * bytes, so [channel][plane][H][W] arrays and the channel stack's interleaved
 * [site][h][w][slot] layout are both read in place (the caller owns every
 * element the strides reach).  dev_rows [n_planes][max_label + 1][n_channels].
 * dev_object_rows NULL: a negative label or a label above max_label is
 * TMH_EINVAL with dev_rows untouched, found as tmh_object_table_device finds
 * it (computed and waited for first).  dev_object_rows = what
 * tmh_object_table_device wrote for the same planes and max_label: the range
 * counts as checked and the planes are not read for it again; either way the
 * kernel never writes for a label outside [0, max_label].  TMH_EINVAL by
 * name: n_channels outside 1..TMH_INTENSITY_MAX_CHANNELS, elem_bytes other
 * than 1 or 2, more than 65,535 planes, a negative stride, dev_pixels not
 * aligned to elem_bytes, dev_rows overlapping an input.  n_planes = 0 does
 * nothing.  Queued on `stream` (NULL: the default stream). */
int tmh_intensity_table_device(const int32_t* dev_labels, const void* dev_pixels, int elem_bytes,
                               int64_t n_planes, int height, int width, int n_channels,
                               int64_t channel_stride, int64_t plane_stride, int64_t row_stride,
                               int64_t pix_stride, int32_t max_label,
                               const tmh_object_row* dev_object_rows, tmh_intensity_row* dev_rows,
                               void* stream);
/* dev_features f64 [n_groups][max_label + 1][n_channels][5]: max, mean, min,
 * sum, std of the objects of each group of n_planes / n_groups consecutive
 * planes (the z-planes of a time point are one 3-D object: their rows are
 * merged first, empty rows skipped); NaN where the merged n is 0.  n_groups
 * must divide n_planes.  Queued on `stream` (NULL: the default stream). */
int tmh_intensity_features_device(const tmh_intensity_row* dev_rows, int64_t n_planes,
                                  int64_t n_groups, int32_t max_label, int n_channels,
                                  double* dev_features, void* stream);
/* Host buffers, pixels in the plain layout [n_channels][n_planes][height]
 * [width].  *max_label = the largest label of all planes; host_rows holds
 * row_capacity rows, n_planes * (*max_label + 1) * n_channels needed: a smaller
 * capacity (or host_rows NULL) is TMH_EINVAL with *max_label set and nothing
 * written.  A negative label: TMH_EINVAL. */
int tmh_intensity_table(const int32_t* host_labels, const void* host_pixels, int elem_bytes,
                        int64_t n_planes, int height, int width, int n_channels,
                        int32_t* max_label, tmh_intensity_row* host_rows, int64_t row_capacity);
int tmh_intensity_features(const tmh_intensity_row* host_rows, int64_t n_planes, int64_t n_groups,
                           int32_t max_label, int n_channels, double* host_features);

/* Input, SegmentationImage.create_from_polygons (tmlib/image.py:740-776) for
 * every plane of a site in one call: the label planes of stored outlines.
 * points is int32 [n_points][2], the rings' vertices one after the other as
 * global map (x, y) pairs (exteriors only: the reference ignores holes, so
 * they are filled); ring p is points first[p] .. first[p + 1] (int64
 * [n_polygons + 1]) and is drawn with label[p] into plane plane[p] (int32
 * [n_polygons] each).  The rings of one plane follow each other in the order
 * of the reference's list: where two overlap, the one later in the arrays
 * wins.  On load xs = x - x_offset and ys = -y - y_offset; the pixels of a
 * ring are those skimage.draw.polygon of scikit-image 0.13.0 gives for (ys,
 * xs) on a height x width plane (an even-odd test against every edge, exact
 * for integer vertices; a repeated closing vertex changes nothing, a ring of
 * one or two vertices fills nothing).  planes_out is int32
 * [n_planes][height][width], zeroed by the call; any int32 label is written
 * as given.  The bit rows of a ring's clipped bounding box (height of the box
 * x ceil(width of the box / 64) words) sit in LDS up to TMH_POLYGON_LDS_WORDS
 * words; a larger box is drawn through a workspace in memory: the same
 * result.  The same input gives the same bytes on every run.
 * TMH_EINVAL with nothing written: an empty ring, first not monotone (or
 * first[0] < 0), a plane index outside 0 .. n_planes - 1, a transformed
 * coordinate of magnitude 2^24 or more, planes_out overlapping an input, more
 * than 65,535 planes, 2^31 - 1 rings or more.  n_polygons = 0 gives zero
 * planes.  The device form reads the lists on `stream` (NULL: the default
 * stream) to check them, waits, then queues the work there and returns when
 * the planes are complete. */
#define TMH_POLYGON_LDS_WORDS 512
int tmh_polygon_fill_device(const int32_t* dev_points, const int64_t* dev_first,
                            const int32_t* dev_plane, const int32_t* dev_label,
                            int64_t n_polygons, int64_t n_planes, int height, int width,
                            int64_t y_offset, int64_t x_offset, int32_t* dev_planes_out,
                            void* stream);
int tmh_polygon_fill(const int32_t* host_points, const int64_t* host_first,
                     const int32_t* host_plane, const int32_t* host_label, int64_t n_polygons,
                     int64_t n_planes, int height, int width, int64_t y_offset, int64_t x_offset,
                     int32_t* host_planes_out);

/* ---- the clustering tool -------------------------------------------------
 * tmlib/tools/clustering.py:40-99 through Classifier.train_unsupervised /
 * predict (tmlib/tools/base.py:586-645): RobustScaler(quantile_range=(1, 99))
 * and KMeans on a feature table.  x is row-major [n][d] f64 (DataFrame.values);
 * all arithmetic is f64.  1 <= d <= TMH_CLUSTER_MAX_D, 1 <= k <=
 * TMH_CLUSTER_MAX_K, k * d <= TMH_CLUSTER_MAX_KD (the centres fit in 64 KB of
 * LDS), n < 2^31; anything larger is TMH_EINVAL.  Fit and seed pick k rows
 * as centres and need k <= n; predict labels any number of rows.  center / scale [d]
 * (both NULL: none) are applied as (x - center) / scale -- one subtract, one
 * divide -- while a kernel loads x: the result is what the same call gives on
 * the array tmh_robust_scale writes, bit for bit.  No sum is decided by a
 * floating-point atomic: the same input gives the same bytes on every run.
 * Every call returns when its host outputs are filled; `stream` (NULL: the
 * default stream) carries the work.  The _device forms take x (and center,
 * scale, labels, min_dist, out) in device memory, the host forms in host
 * memory; small tables (ranks, draws, centres, counts) are host memory in both. */
#define TMH_CLUSTER_MAX_D 256
#define TMH_CLUSTER_MAX_K 64
#define TMH_CLUSTER_MAX_KD 8192
#define TMH_CLUSTER_MAX_RANKS 64
#define TMH_CLUSTER_MAX_TRIALS 16
/* Per column: host_count = values that are not NaN, host_inf = values that are
 * +-inf; host_mean / host_var (each may be NULL) = mean and variance of the
 * scaled column over its non-NaN values, np.var's definition (two passes,
 * divisor = the count), summed in a fixed order. */
int tmh_column_census_device(const double* dev_x, int64_t n, int d, const double* dev_center,
                             const double* dev_scale, int64_t* host_count, int64_t* host_inf,
                             double* host_mean, double* host_var, void* stream);
int tmh_column_census(const double* host_x, int64_t n, int d, const double* host_center,
                      const double* host_scale, int64_t* host_count, int64_t* host_inf,
                      double* host_mean, double* host_var);
/* host_values[f][q] = the value at 0-based rank host_ranks[f][q] among column
 * f's non-NaN values in ascending order, exactly (a radix select on the
 * order-preserving 64-bit image of the f64; -0.0 sorts below +0.0, the two are
 * equal as values).  1 <= r <= TMH_CLUSTER_MAX_RANKS; a rank outside the
 * column's non-NaN count: TMH_EINVAL.  host_count [d]: the non-NaN counts
 * tmh_column_census returned for the same x, against which the ranks are
 * checked (with a count above the column's true one, a rank past the true
 * count returns NaN; nothing is read out of bounds); NULL: the call takes a
 * census of its own, one more read of x. */
int tmh_column_select_device(const double* dev_x, int64_t n, int d, const int64_t* host_count,
                             const int64_t* host_ranks, int r, double* host_values, void* stream);
int tmh_column_select(const double* host_x, int64_t n, int d, const int64_t* host_count,
                      const int64_t* host_ranks, int r, double* host_values);
/* out = (x - center) / scale (RobustScaler.transform); x and out must not overlap. */
int tmh_robust_scale_device(const double* dev_x, int64_t n, int d, const double* dev_center,
                            const double* dev_scale, double* dev_out, void* stream);
int tmh_robust_scale(const double* host_x, int64_t n, int d, const double* host_center,
                     const double* host_scale, double* host_out);
/* k-means++ as scikit-learn's _kmeans_plusplus states it.  `first` is the
 * first centre's row; host_draws [k - 1][trials] are the uniform draws of each
 * step (trials = 2 + int(log(k)) for scikit-learn's choice, at most
 * TMH_CLUSTER_MAX_TRIALS).  Per step: target = draw * current potential; the
 * candidate is the first row whose inclusive prefix sum of the closest squared
 * distances reaches the target (at most n - 1); the trial with the smallest
 * potential is kept (the first of equals).  host_indices [k], host_centers
 * [k][d] (scaled).  host_trace (may be NULL) [k - 1][3 * trials + 1] doubles:
 * per step the targets, the candidate rows, the potentials, the kept trial.
 * The k-means calls return TMH_EINVAL when x holds NaN or +-inf. */
int tmh_kmeans_seed_device(const double* dev_x, int64_t n, int d, int k, const double* dev_center,
                           const double* dev_scale, int64_t first, const double* host_draws,
                           int trials, int32_t* host_indices, double* host_centers,
                           double* host_trace, void* stream);
int tmh_kmeans_seed(const double* host_x, int64_t n, int d, int k, const double* host_center,
                    const double* host_scale, int64_t first, const double* host_draws, int trials,
                    int32_t* host_indices, double* host_centers, double* host_trace);
/* labels[i] = argmin_j sum_f (x_if - c_jf)^2, summed in feature order, the
 * first minimum; min_dist (may be NULL) [n] = that minimum.  x must not
 * overlap labels or min_dist. */
int tmh_kmeans_predict_device(const double* dev_x, int64_t n, int d, int k, const double* dev_center,
                              const double* dev_scale, const double* host_centers,
                              int32_t* dev_labels, double* dev_min_dist, void* stream);
int tmh_kmeans_predict(const double* host_x, int64_t n, int d, int k, const double* host_center,
                       const double* host_scale, const double* host_centers, int32_t* host_labels,
                       double* host_min_dist);
/* Lloyd's iterations from host_init [k][d] as scikit-learn's
 * _kmeans_single_lloyd runs them.  *tol_abs = tol * the mean of the scaled
 * columns' variances.  An iteration assigns, then moves the centres; an empty
 * cluster (ascending index) takes the row farthest from its own centre (ties:
 * the lowest row; rows in descending distance), which leaves its old cluster.
 * The loop stops when no label changed or when the summed squared centre shift
 * is <= *tol_abs; unless it stopped on unchanged labels one more assign makes
 * the labels those of the final centres.  *n_iter counts as n_iter_ does. */
int tmh_kmeans_fit_device(const double* dev_x, int64_t n, int d, int k, const double* dev_center,
                          const double* dev_scale, const double* host_init, int max_iter, double tol,
                          double* host_centers, int32_t* dev_labels, double* inertia, int* n_iter,
                          double* tol_abs, void* stream);
int tmh_kmeans_fit(const double* host_x, int64_t n, int d, int k, const double* host_center,
                   const double* host_scale, const double* host_init, int max_iter, double tol,
                   double* host_centers, int32_t* host_labels, double* inertia, int* n_iter,
                   double* tol_abs);

/* ---- the supervised classification tool ------------------------------------
 * tmlib/tools/classification.py:45-116 through Classifier.predict
 * (tmlib/tools/base.py:621-645): the labels scikit-learn's
 * RandomForestClassifier.predict and SVC.predict give, from a flat model that
 * the Python layer exports from the fitted estimator.  Training is not here.
 * x is row-major [n][d] f64, 1 <= d <= TMH_CLUSTER_MAX_D, n < 2^31; x holding
 * NaN or +-inf is TMH_EINVAL.  The _device forms take x (and center, scale,
 * labels, proba, dec) in device memory, the host forms in host memory; the
 * model arrays of the create calls are host memory.  Every predict returns
 * when its work is done; x must not overlap an output, nor labels the other
 * output (TMH_EINVAL).
 *
 * Forest (RandomForestClassifier.predict of scikit-learn 1.7.2).  x is cast to
 * float32, round to nearest even; a finite value whose cast is infinite is
 * TMH_EINVAL.  At a node the row goes left iff (double)x_f32[feature] <=
 * threshold.  A leaf contributes its row of leaf_value (fractions, not
 * renormalised).  The trees' rows are added in f64 in tree order into zero,
 * each class sum is divided by n_trees once, the label is the first maximum:
 * labels and proba [n][n_classes] (may be NULL) equal scikit-learn's exactly.
 *
 * The model: feature [nodes] (-1: a leaf), threshold [nodes], left / right
 * [nodes], leaf_row [nodes] (a leaf's row of leaf_value), tree_root [n_trees]
 * (ascending from 0; a tree owns the nodes from its root up to the next
 * tree's), leaf_value [n_leaves][n_classes].  2 <= n_classes <=
 * TMH_FOREST_MAX_CLASSES, 1 <= n_trees <= TMH_FOREST_MAX_TREES, nodes <
 * TMH_FOREST_MAX_NODES.  tmh_forest_create checks before anything is
 * uploaded, TMH_EINVAL otherwise: an internal node's children lie inside its
 * tree and have indices greater than its own (so every walk ends), no node is
 * reached twice, feature < d, no threshold is NaN, every leaf_row is in range,
 * the leaf values are finite.
 *
 * Two routes, chosen by the model alone (tmh_forest_route): packed nodes
 * (16 bytes each, the nodes a root reaches) that fit 96 KB are staged into
 * LDS once per workgroup (TMH_FOREST_ROUTE_LDS), a larger forest is walked in
 * memory (TMH_FOREST_ROUTE_MEMORY).  TMH_OPT_FOREST_MEMORY_ROUTE = 1 forces
 * the memory route.  Both give the same bytes. */
#define TMH_FOREST_MAX_CLASSES 64
#define TMH_FOREST_MAX_TREES 256
#define TMH_FOREST_MAX_NODES (1 << 24)
#define TMH_FOREST_ROUTE_LDS 0
#define TMH_FOREST_ROUTE_MEMORY 1
#define TMH_OPT_FOREST_MEMORY_ROUTE 20
typedef struct tmh_forest tmh_forest;
int tmh_forest_create(const int32_t* feature, const double* threshold, const int32_t* left,
                      const int32_t* right, const int32_t* leaf_row, int64_t nodes,
                      const int32_t* tree_root, int n_trees, const double* leaf_value,
                      int64_t n_leaves, int n_classes, int d, tmh_forest** out);
void tmh_forest_destroy(tmh_forest* h);
int tmh_forest_set_option(tmh_forest* h, int option, int value);
/* *route = the route a predict takes now; *packed_nodes (may be NULL) */
int tmh_forest_route(const tmh_forest* h, int* route, int64_t* packed_nodes);
int tmh_forest_predict_device(tmh_forest* h, const double* dev_x, int64_t n, int32_t* dev_labels,
                              double* dev_proba, void* stream);
int tmh_forest_predict(tmh_forest* h, const double* host_x, int64_t n, int32_t* host_labels,
                       double* host_proba);
/* SVC (libsvm's dense svm_predict_values as scikit-learn 1.7.2 ships it).
 * center / scale [d] (both NULL: none) are applied as (x - center) / scale on
 * load, as the clustering calls do.  K_s = exp(-gamma sum_f (x_f - sv_sf)^2)
 * (TMH_SVC_RBF, the differenced form) or x . sv_s (TMH_SVC_LINEAR).  For each
 * class pair (i < j) in libsvm's order (0,1), (0,2), ..., (1,2), ...:
 *   dec = sum over the SVs of i of coef[j - 1][s] K_s
 *       + sum over the SVs of j of coef[i][s] K_s - rho[p];
 * the vote goes to i iff dec > 0, else to j; the label is the class with the
 * most votes, the first on equality.  All arithmetic is f64; the sums run in
 * ascending s as fused multiply-adds (libsvm's go through BLAS, whose order is
 * free), so dec agrees with libsvm's within rounding, not bit for bit.  dec
 * [n][k (k - 1) / 2] may be NULL.  A linear model is collapsed at create to
 * one weight vector per pair.
 *
 * The model, in libsvm's own sign convention (scikit-learn's _dual_coef_ and
 * -_intercept_, not the public attributes): sv [m][d] grouped by class, n_sv
 * [k] adding up to m, coef [k - 1][m], rho [k (k - 1) / 2]; gamma > 0 for rbf.
 * 2 <= k <= TMH_SVC_MAX_CLASSES, 1 <= m <= TMH_SVC_MAX_SV; every value
 * finite; anything else is TMH_EINVAL.  The support vectors stream through LDS
 * in tiles (tmh_svc_tile: SVs per tile, number of tiles); TMH_OPT_SVC_TILE
 * caps the tile (0: no cap).  Every tile size gives the same bytes. */
#define TMH_SVC_RBF 0
#define TMH_SVC_LINEAR 1
#define TMH_SVC_MAX_CLASSES 16
#define TMH_SVC_MAX_SV 65536
#define TMH_OPT_SVC_TILE 21
typedef struct tmh_svc tmh_svc;
int tmh_svc_create(int kernel, double gamma, const double* sv, int64_t m, int d, const int32_t* n_sv,
                   int k, const double* coef, const double* rho, tmh_svc** out);
void tmh_svc_destroy(tmh_svc* h);
int tmh_svc_set_option(tmh_svc* h, int option, int value);
int tmh_svc_tile(const tmh_svc* h, int* tile, int* n_tiles);
int tmh_svc_predict_device(tmh_svc* h, const double* dev_x, int64_t n, const double* dev_center,
                           const double* dev_scale, int32_t* dev_labels, double* dev_dec,
                           void* stream);
int tmh_svc_predict(tmh_svc* h, const double* host_x, int64_t n, const double* host_center,
                    const double* host_scale, int32_t* host_labels, double* host_dec);

/* ---- device memory helpers for callers without another allocator -------- */
int tmh_malloc_device(void** dev_ptr, size_t bytes);
int tmh_free_device(void* dev_ptr);
int tmh_memcpy(void* dst, const void* src, size_t bytes, int kind /*0 h2d,1 d2h,2 d2d*/,
               void* stream);

/* ---- timing of the most recent launches (bench/roofline support) ---------
 * Per-kernel event timing on the handle's stream, enabled by flag. */
int tmh_profile_enable(int on);
int tmh_profile_read(const char* kernel, double* total_ms, int64_t* launches);
int tmh_profile_reset(void);

#ifdef __cplusplus
}
#endif
#endif /* TMHIP_H */
