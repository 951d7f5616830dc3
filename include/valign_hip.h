/*
 * valign_hip.h -- entry points of libHIPKernel.so, the MI355X (gfx950) backend.
 *
 * (1) The versalignLib plugin boundary -- what the reference host binds with dlsym()
 *     (src/util/versalignUtil.cpp:35-76, src/impl/main.cpp:217-238).  Same four symbols
 *     and the same behaviour as src/Kernels/default/DefaultKernel_dllexport.cpp:18-42:
 *
 *       AlignmentKernel *spawn_alignment_kernel();
 *       void set_parameters(AlignmentParameters *);
 *       void set_logger(AlignmentLogger *);
 *       void delete_alignment_kernel(AlignmentKernel *);
 *
 *     The spawned object implements AlignmentKernel::score_alignments and
 *     ::compute_alignments (include/AlignmentKernel.h:40-43, restated in
 *     versalign_plugin_abi.h).  Required parameter keys are the reference's six
 *     (DefaultKernel.h:70-75); a missing one makes spawn throw the same C string.
 *     Optional keys, probed with has_key (a reference host simply lacks them):
 *       score_gap_open_read / score_gap_extend_read /
 *       score_gap_open_ref  / score_gap_extend_ref ... affine-gap extension (scores and alignments)
 *       traceback_policy ................................ 0 Default/OpenCL tie-breaks (default),
 *                                                         1 SSE2/AVX2 tie-breaks (linear gaps)
 *       band_width ...................................... > 0: banded Smith-Waterman scores, that
 *                                                         many diagonals around the main one (strip band)
 *       band_alignments ................................. 1: compute_alignments under band_width > 0 returns banded
 *                                                         Smith-Waterman alignments on the scores' block band;
 *                                                         0 (default): every cell whatever band_width says
 *                                                         (opt-in: existing calls return what they did)
 *       band_nw ......................................... 1: band_width > 0 also applies to the scores of the NW variant
 *                                                         and, with band_alignments = 1, to its alignments (definition at
 *                                                         valign_hip_set_band_nw); 0 (default): both are refused under a
 *                                                         band.  Smith-Waterman calls are untouched.  Other values are refused
 *       trace_checkpoints ............................... 1: compute_alignments of long reads (the plain row strips: unbanded,
 *                                                         int16 cells, traceback_policy 0) keeps one boundary row per strip
 *                                                         and ONE strip's pointers and re-fills strip after strip along the
 *                                                         walk: identical alignments, 5.5 instead of 51.5 MB of scratch per
 *                                                         pair of pairs at 10 kbp x 10 kbp; 0 (default): every pointer
 *       score_width ..................................... DP cells of score_alignments: 0 auto (int16,
 *                                                         int32 where int16 could overflow), 16, 32
 *       ragged_batching ................................. length-sorted score calls, both modes
 *                                                         (trailing non-ACGT padding is not swept,
 *                                                         identical scores): 0 never (default), 1 when a
 *                                                         sample of the call is ragged enough, 2 always
 *       host_malloc_tuning .............................. 0 (default): the plugin leaves the HOST's allocator alone.
 *                                                         A host that wants compute_alignments' 2n operator new[]
 *                                                         result rows cheap (~50 ms instead of ~700 ms per million
 *                                                         pairs with 16 threads) starts with MALLOC_TOP_PAD_=268435456
 *                                                         in its environment -- or sets this key:
 *                                                         2 = mallopt(M_TOP_PAD, 256 MB) from the plugin (process-wide,
 *                                                         logged at WARNING level the first time), 1 = that +
 *                                                         M_TRIM_THRESHOLD off.  Other values are refused.
 *       host_packing .................................... score_alignments: 1 (default) sequences cross PCIe as 4-bit
 *                                                         base classes (identical scores), 0 raw ASCII
 *       half_float_cells ................................ score_alignments: 1 (default) half-float cells where they are
 *                                                         exact (identical scores, fewer instructions), 0 integer cells
 *       pointer_scratch_cap_mb .......................... cap of compute_alignments' device-side pointer
 *                                                         scratch in MiB (default 0: 64 GiB / half the free HBM)
 *       hip_device ...................................... device ordinal (default 0)
 *       hip_devices ..................................... N > 1: every call is split into N contiguous shards of
 *                                                         pairs, one per device (hip_device .. hip_device+N-1,
 *                                                         modulo the visible ones -- folding is announced at
 *                                                         WARNING level), each on its own host thread;
 *                                                         results land in the caller's arrays (default 1)
 *       hip_devices_strict .............................. 1: refuse hip_devices beyond the visible devices
 *       hip_devices_allgather ........................... 1: score_alignments keeps every shard's scores on its device and
 *                                                         runs an RCCL all-gather over them (librccl.so, loaded with dlopen;
 *                                                         one communicator per device in this process): the whole score
 *                                                         vector ends up on every device, the host copy comes from the
 *                                                         first.  Needs one distinct device per shard.  Default 0: every
 *                                                         shard copies its own scores to the host, no collective
 *       hip_group_lanes / hip_rows_per_lane ............. force a kernel geometry
 *
 * (2) A flat C view of the same engine for callers that already hold the batch in
 *     device memory (bench.py, multi-GPU sharding): plain pointers and sizes only.
 *     These replace nothing in the reference -- its OpenCL backend is the closest
 *     precedent (gather -> contiguous pair-major buffers -> device,
 *     src/Kernels/OpenCL/OpenCLKernel.cpp:57-108) -- and take exactly the contiguous
 *     buffers that backend builds internally.
 *
 * All flat functions return 0 on success, non-zero on failure (message through
 * valign_hip_last_error()).  There is no CPU fallback anywhere in this library.
 */
#ifndef VALIGN_HIP_H
#define VALIGN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- (1) plugin boundary (C++ types from versalign_plugin_abi.h) ---- */
#ifdef __cplusplus
class AlignmentKernel;
class AlignmentParameters;
class AlignmentLogger;
AlignmentKernel *spawn_alignment_kernel();
void set_parameters(AlignmentParameters *parameters);
void set_logger(AlignmentLogger *logger);
void delete_alignment_kernel(AlignmentKernel *instance);
#endif

/* ---- (2) flat device-resident API ---- */
typedef struct valign_hip_engine valign_hip_engine;

typedef struct {
    int32_t match, mismatch;          /* score_match, score_mismatch                      */
    int32_t gap_read, gap_ref;        /* score_gap_read (LEFT), score_gap_ref (UP)        */
    int32_t affine;                   /* 0: linear model above; 1: use the four below     */
    int32_t open_read, ext_read;      /* first / further gap base in the read (LEFT)      */
    int32_t open_ref, ext_ref;        /* first / further gap base in the ref  (UP)        */
} valign_hip_scoring;

int valign_hip_device_count(void);

/* Plugin key hip_devices = N: shard d (0-based) of a call of n pairs is the contiguous range [*begin, *begin + *count)
 * -- ceil(n / N) pairs per shard, the last one short, trailing shards empty.  Pure arithmetic (no device needed): the one
 * rule the shard threads and the in-plugin all-gather's buffer offsets both use.  Returns 1 on bad arguments.            */
int valign_hip_shard_range(int n, int shards, int d, int *begin, int *count);

/* One engine = one device + fixed (read_length, ref_length, scoring), like one spawned
 * kernel object.  force_group_lanes / force_rows_per_lane = 0 lets the engine choose. */
int valign_hip_engine_create(int device, int read_length, int ref_length,
                             const valign_hip_scoring *scoring, int force_group_lanes,
                             int force_rows_per_lane, valign_hip_engine **out);
void valign_hip_engine_destroy(valign_hip_engine *e);

/* Tie-break rules of compute_alignments: 0 = the reference's Default/OpenCL kernels (default),
 * 1 = its SSE2/AVX2 kernels (DIAG only between ACGT bases > LEFT > UP, no stop at zero cells,
 * N invalid for the NW end cell; src/Kernels/AVX-SSE/SSEKernel.cpp:366-379, 532-536).          */
int valign_hip_set_traceback_policy(valign_hip_engine *e, int policy);

/* Banded Smith-Waterman scores (an extension: the reference has no banding).  Definition, w = diagonals / 2:
 * the per-cell band is |j - floor(i * ref_length / read_length)| <= w (i, j 0-based read / ref positions).
 * The library computes AT LEAST that band: the read's rows are taken in blocks of B consecutive rows (the last
 * block ends with the last row), and a block computes the columns [floor(r_first * F / R) - w,
 * floor(r_last * F / R) + w] of its rows r_first..r_last, the lower end rounded down to a multiple of A; every
 * other cell counts as 0 and cannot hold the maximum.  Hence  score(per-cell band w) <= result <= score(all
 * cells),  and the result equals this block definition exactly (oracle/cpu_ref.c, vref_score_banded_sw[_affine],
 * restates it with B and A as parameters; B = 1 / A = 1 is the per-cell band).
 *
 * WHICH (B, A) applies depends on the schedule the engine can use for (shape, band, scoring), and
 * valign_hip_describe is the authority -- "band_block_rows" / "band_col_align" of the engine after
 * valign_hip_set_band_width:
 *   B = 16,  A = 1   the cyclic block chain (band_kernels.hip.h): linear gaps since round 3, affine gaps since round 4,
 *                    wherever its plan fits (windows up to 2048 columns of reference ring, delays up to 64 steps);
 *                    exported below as VALIGN_HIP_BAND_CHAIN_BLOCK_ROWS / VALIGN_HIP_BAND_CHAIN_COL_ALIGN;
 *   B = 160, A = 4   row strips (long_kernels.hip.h): every other banded case; VALIGN_HIP_BAND_BLOCK_ROWS /
 *                    VALIGN_HIP_BAND_COL_ALIGN.
 * The chain's band is the tighter superset of the per-cell band.  0 (default) computes every cell; a band wider
 * than the matrix gives the unbanded result.
 *
 * Alignments use the SAME block band once valign_hip_set_band_alignments(e, 1) (key band_alignments = 1) is set:
 * the reference's Default SW fill and traceback (DefaultKernel.cpp:204-280, 391-456) on int32 semantics, every cell
 * outside the band 0 with pointer START (affine gaps: H = E = F = 0), the end cell the row-major first strict maximum
 * over in-band cells, the walk ending at START or at a step that leaves the band.  So the score of every returned
 * alignment is the banded score of the same pair, and a band of at least 2 * max(R, F) gives the unbanded alignments.
 * Smith-Waterman with linear or affine gaps and traceback_policy = 0 only: NW alignments and traceback_policy = 1 are
 * refused under band_alignments = 1.                                                                             */
#define VALIGN_HIP_BAND_BLOCK_ROWS 160
#define VALIGN_HIP_BAND_COL_ALIGN 4
#define VALIGN_HIP_BAND_CHAIN_BLOCK_ROWS 16
#define VALIGN_HIP_BAND_CHAIN_COL_ALIGN 1
int valign_hip_set_band_width(valign_hip_engine *e, int diagonals);
/* 1: valign_hip_align_device / _align_host return banded SW alignments when band_width > 0 (above); 0 (default):
 * unbanded alignments whatever band_width says.  Other values are refused.                                       */
int valign_hip_set_band_alignments(valign_hip_engine *e, int on);

/* The band for the reference's Needleman-Wunsch variant (key band_nw; the mode that places a whole read inside a reference
 * window: the read is consumed end to end, the reference ends are free).  0 (default): NW-variant scores under band_width > 0
 * and NW-variant alignments under band_alignments = 1 are refused, as ever.  1: band_width > 0 also applies to NW-variant
 * scores and, together with band_alignments = 1, to NW-variant alignments (linear and affine gaps; traceback_policy = 1 stays
 * refused under a band).  Smith-Waterman calls do not read the key.  DEFINITION -- windows exactly those of the Smith-Waterman
 * band: row i (0-based read position) has the inclusive column window [lo_i, hi_i] of its block, on the (B, A) that
 * valign_hip_describe reports after valign_hip_set_band_width ((16, 1) on the chain, (160, 4) on strips; band_window.h):
 *   - a cell (i, j) with j outside [lo_i, hi_i] is ABSENT: never a candidate of a neighbour, never part of a maximum or an
 *     arg-max; with affine gaps H, E and F are all absent there;
 *   - the border row above read row 0 is present at every column, value 0, pointer START; the border column left of ref
 *     column 0 is present at row i only where lo_i == 0, with the unbanded values: scores 0; alignments (i + 1) * gap_ref with
 *     pointer UP (linear gaps), open_ref + i * ext_ref entered from F (affine gaps);
 *   - present cells use the unbanded NW-variant recurrence and tie-breaks: DIAG > UP > LEFT (linear gaps); Gotoh with
 *     DIAG > F > E and a gap opened rather than extended on ties (affine gaps);
 *   - the score is max(0, present cells of the last read row, present cells of the last ref column);
 *   - the alignment's end cell follows the reference's rule on present cells: end_i is the last row before the first invalid
 *     read byte, end_j = min(last_ref, arg), arg the first strict arg-max over the present cells of row end_i, the running
 *     best starting at the border column's value where lo == 0 and at absent otherwise.  Where that start cell is absent
 *     (say last_ref < lo) the alignment is empty: all-zero rows, the four coordinates R + F - 1, an all-zero CIGAR record;
 *   - calls with 2 * (band_width / 2) + 1 < ceil(F / R) are refused: the windows of consecutive blocks would not connect.  In
 *     every accepted call each in-band cell has a present candidate, so a pointer never leads out of the band.
 * Hence a band of at least 2 * max(R, F) gives exactly the unbanded NW-variant scores and alignments, and for scores
 * per-cell band <= block band <= unbanded.  Scores run on int32 cells; alignments on the packed int16 strips where the
 * sentinel that stands for "absent" is provably safe (band_nw_int16_ok, cell_rules.h), else on int32 cells
 * ("ran_align_fill": strip_band / strip_wide_band).  tests/band_nw_ref.py restates the definition in numpy.  Other values
 * than 0 / 1 are refused.                                                                                         */
int valign_hip_set_band_nw(valign_hip_engine *e, int on);

/* Checkpointed traceback for long-read alignments in bounded memory (key trace_checkpoints).  Reads beyond one register sweep
 * are filled in row strips of 64 K rows, and by default (0) every strip streams 2 bits per cell and pair (4 with affine gaps) to
 * a pointer region of its own: S regions, memory that grows with R x F.  With 1, calls that take the plain row strips --
 * unbanded, int16 cells, traceback_policy = 0; Smith-Waterman and the NW variant, linear and affine gaps, both entry paths and
 * every hip_devices shard -- run a forward pass that stores NO pointers and keeps every strip's bottom row (S - 1 boundary rows
 * per pair of pairs instead of the two that ping-pong), then walk back strip by strip, last to first: the strip is filled again,
 * with pointers, into ONE strip-sized region that every round reuses (from the checkpoint row above it, and only up to the
 * column the walk has reached), and the walk crosses it and leaves its state for the next round.  The alignments are
 * bit-identical; the scratch per pair of pairs is one region + (S - 1) rows + 48 bytes of walk state (10 kbp x 10 kbp at 16
 * rows per lane: 5.5 MB instead of 51.5 MB, linear gaps), so a given pointer_scratch_cap_mb holds nine times the pairs.
 * Not covered, and run exactly as with 0: int32 cells (strip_wide), bands (strip_band, strip_wide_band), traceback_policy = 1
 * and the register and fused paths of short reads -- the key saves memory and changes no result, so nothing is refused;
 * "ran_align_fill" of valign_hip_describe says which path ran ("strip_ckpt" for this one), "align_ptr_bytes_per_pair" and
 * "align_ckpt_bytes_per_pair" what a pair holds (pointers; checkpoint rows + walk state), "align_scratch_bytes" what the
 * engine holds after the call.  Values other than 0 and 1 are refused.
 * Time, measured at 10 kbp x 10 kbp against the full-pointer path (profiles/r07_trace_checkpoints.txt): with linear gaps a
 * call whose full pointer scratch fits the device in one piece is SLOWER with the key -- 4,096 pairs: 143.7 against 137.6 ms
 * (SW), 131.1 against 120.6 ms (NW variant), 1.04 x / 1.09 x -- because every cell is filled one and a half times; the key is
 * there for the memory bound.  Where the full-pointer path has to run in chunks it is faster: affine gaps 201 against 329 ms
 * (4,096 pairs), 16,384 pairs 661 against 835 ms (linear) and 903 against 1,322 ms (affine).                                 */
int valign_hip_set_trace_checkpoints(valign_hip_engine *e, int on);

/* Cap (MiB) of the internal pointer scratch compute_alignments keeps in device memory (2 bits per cell and pair,
 * 4 with affine gaps: 20.8 / 41.6 KB per pair at 150 x 500).  0 (default): up to 64 GiB or half the free HBM,
 * whichever is smaller; batches that need more than the cap run in chunks -- same results, more launches.
 * Plugin key: pointer_scratch_cap_mb.                                                                       */
int valign_hip_set_pointer_scratch_cap_mb(valign_hip_engine *e, long long mb);

/* DP cell width of the score path: 0 (default) = int16 like the reference, switching to int32 cells
 * for (shape, scoring, mode) whose cells could leave int16 (the reference would wrap silently);
 * 16 = int16 or refuse; 32 = always int32 (strip path, one pair per register: half the rate).
 * Scores beyond the ABI's short saturate at 32767.                                               */
int valign_hip_set_score_width(valign_hip_engine *e, int bits);

/* Length-sorted batching of score calls (Smith-Waterman and the NW variant; valign_hip_score_host / score_alignments
 * and valign_hip_score_device): the reference host pads every sequence to the longest
 * (src/util/versalignUtil.cpp:17-33) and every backend sweeps the padding; here pairs are binned by their length
 * without trailing non-ACGT bytes and each bin is swept at its own shape.  Scores are identical: trailing padding
 * scores 0, so it cannot raise a Smith-Waterman maximum, and every value of the real matrix's last row / column runs
 * down its diagonal unchanged to the padded matrix's, which is where the NW variant reads its result.
 * Classification, packing by length class and the scores' way back run on the device.  0 = never (default), 1 = when the
 * call is ragged enough to skip a third of the cells (host pointers: judged from a sample of the call's tails;
 * valign_hip_score_device: from the device's histogram), 2 = always.  With mode 1 or 2 valign_hip_score_device WAITS
 * for the classification of the batch before it launches the sweeps (the rest is asynchronous on `stream` as ever)
 * and uses scratch of the engine: such calls on one engine go on one stream at a time.                        */
int valign_hip_set_ragged_batching(valign_hip_engine *e, int mode);

/* Score n pairs that are already in device memory: d_reads = n*read_length bytes and
 * d_refs = n*ref_length bytes (raw ASCII, pair-major, NUL padded), d_scores = n int16.
 * opt & 0xF: 0 Smith-Waterman, 1 Needleman-Wunsch variant; other values do nothing.
 * Asynchronous on `hip_stream` (a hipStream_t; NULL = the device's default stream).    */
int valign_hip_score_device(valign_hip_engine *e, int opt, long long n, const void *d_reads,
                            const void *d_refs, void *d_scores, void *hip_stream);

/* Align n device-resident pairs (linear gaps: the reference's model, Default-kernel tie-breaks;
 * affine scoring: the Gotoh extension, same tie-breaks where they apply): d_rows = n * 2 * (R+F) bytes,
 * per pair the read row then the ref row -- right-justified gapped strings in
 * [start, R+F-2], zeros before start, NUL at R+F-1 -- and d_idx = n * 4 int16
 * (readStart, readEnd, refStart, refEnd), i.e. the contents of the ABI's `Alignment`
 * (include/AlignmentKernel.h:12-18) flattened.  Tie-breaks follow the Default kernel.
 * Asynchronous on `hip_stream`; uses an internal pointer scratch (20.8 KB per pair at
 * 150x500, 25 MB at 10 kbp x 10 kbp -- 2.8 MB with valign_hip_set_trace_checkpoints(e, 1); up to half the free HBM per
 * launch -- at most 64 GiB for reads of up to 2048 rows, 128 GiB for row strips --, larger batches run in chunks).   */
int valign_hip_align_device(valign_hip_engine *e, int opt, long long n, const void *d_reads,
                            const void *d_refs, void *d_rows, void *d_idx, void *hip_stream);

/* The plugin virtual without the C++ object: host pointers in, host scores out
 * (gather -> pinned staging -> H2D -> kernel -> D2H, chunked and overlapped).          */
int valign_hip_score_host(valign_hip_engine *e, int opt, int n, const char *const *reads,
                          const char *const *refs, short *scores, int threads);

/* compute_alignments for host pointers into caller-provided contiguous buffers: rows = n * 2 *
 * (read_length + ref_length) bytes (read row, then ref row, per pair; zeros before the start, NUL at
 * the end), idx = n * 4 shorts (readStart, readEnd, refStart, refEnd).  Same results as the plugin's
 * compute_alignments without its 2n operator new[] blocks -- for FFI callers (ctypes, cgo, JNI).      */
int valign_hip_align_host(valign_hip_engine *e, int opt, int n, const char *const *reads,
                          const char *const *refs, void *rows, short *idx, int threads);

/* ---- compact alignment results: placed CIGARs from the device ----
 * A second result format beside the rows: per pair one fixed record and a run of 32-bit ops, encoded ON THE DEVICE behind the
 * traceback, so every alignment path feeds it (fused small calls, the register geometries, row strips, int32 strips, banded
 * strips, checkpointed strips; both traceback policies) and every key of the alignment path applies unchanged.  The rows stay
 * in an engine-owned device scratch (a chunk of the call at a time: "cigar_rows_scratch_bytes") and never cross PCIe.
 *   op ......... length << 4 | code, BAM codes M 0, I 1, D 2, = 7, X 8, in reading order.  Columns are classified exactly as
 *                vh_cigar does (valign_host.h): '-' in the read row is D, '-' in the ref row is I, otherwise M -- or, with
 *                extended = 1, '=' where the two bytes are equal ignoring case and X where not.  The ops rendered as text are
 *                vh_cigar's string of the rows valign_hip_align_device returns for the same pair.  No soft clips and no
 *                N / S / H / P ops: read_begin / read_end say what part of the read is aligned.
 *   coordinates  0-based, half-open, in the read / reference as passed in: the ends are the fill's end cell + 1, the
 *                begins the ends minus the non-gap bases of the rows.  This is what the rows cannot say: WHERE in the
 *                reference a Smith-Waterman alignment lies.
 *   score ...... the returned alignment re-scored under the engine's scoring: match / mismatch between two ACGT bases of
 *                either case, 0 for any other pair of bytes; linear gaps gap_read per '-' in the read row and gap_ref per '-'
 *                in the ref row; affine gaps open + (k - 1) * extend per maximal run of k and direction.  int32, defined for
 *                both algorithms and every path.
 *   empty ...... an empty alignment (Smith-Waterman maximum 0; an NW-variant read that starts with an invalid byte) is
 *                n_ops = 0 with all four coordinates and the score 0.                                                       */
typedef struct {                     /* 24 bytes */
    int32_t read_begin, read_end;
    int32_t ref_begin, ref_end;
    int32_t score;
    uint32_t n_ops;                  /* ops this alignment has (may exceed what was stored, below) */
} valign_hip_aln;

/* Device-resident: asynchronous on hip_stream like valign_hip_align_device, no host round trip.  d_recs = n records,
 * d_ops = n * ops_stride uint32.  A pair stores its first min(n_ops, ops_stride) ops at d_ops + pair * ops_stride; n_ops
 * always says how many there are, so the caller sees an overflow per pair (words past a pair's ops are not written).
 * extended: 0 = M, 1 = '=' / X.  opt & 0xF > 1 does nothing.                                                               */
int valign_hip_align_cigar_device(valign_hip_engine *e, int opt, long long n, const void *d_reads,
                                  const void *d_refs, int extended, void *d_recs, void *d_ops,
                                  int ops_stride, void *hip_stream);

/* Host pointers in, packed results out: recs[n], offsets[n + 1] (offsets[0] = 0), pair p's ops are
 * ops[offsets[p] .. offsets[p + 1]).  The gather -> H2D -> fill -> walk pipeline of valign_hip_align_host with the copy-back
 * replaced: per chunk the device counts, scans and packs, and ONE copy brings the records and the ops back (24 bytes + 4 per op
 * and pair instead of the rows; "cigar_d2h_bytes" of valign_hip_describe).  If the call needs more than ops_cap ops it returns
 * non-zero, *ops_needed holds the total and recs / offsets are complete, so the caller can size the retry exactly (on success
 * *ops_needed = offsets[n]).  n = 0 sets offsets[0] = 0; opt & 0xF > 1 writes nothing.                                      */
int valign_hip_align_cigar_host(valign_hip_engine *e, int opt, int n, const char *const *reads,
                                const char *const *refs, int extended, valign_hip_aln *recs,
                                uint32_t *ops, long long ops_cap, long long *offsets,
                                long long *ops_needed, int threads);

/* ---- placed Smith-Waterman scores: score and end cell without a traceback ----
 * What a mapper asks before it asks for an alignment: how good is the best local alignment of a pair, and WHERE in the
 * reference does it end?  The score sweep answers both -- no pointer stream, no pointer scratch, no walk.
 * For Smith-Waterman (opt & 0xF == 0):
 *   score ....... the value valign_hip_score_device returns for the pair.
 *   read_end, ref_end
 *                 (read_end - 1, ref_end - 1) is the reference's end cell under the Default rules
 *                 (src/Kernels/default/DefaultKernel.cpp:252-256): the first cell in row-major order whose value is strictly
 *                 greater than every earlier one -- of all cells that hold the maximum the one in the earliest read row and,
 *                 within that row, the earliest reference column.  So both are 0-based and half-open, and equal
 *                 valign_hip_aln.read_end / .ref_end of valign_hip_align_cigar_device for the same pair.
 *   empty ....... a pair whose maximum is 0 returns {0, 0, 0}.
 * Placed scores run on int16 cells; ragged_batching and half_float_cells are not read by these calls.  opt & 0xF > 1 does
 * nothing, as everywhere.  NOT BUILT HERE -- each is refused with a non-zero return and a message in valign_hip_last_error:
 *   opt & 0xF == 1 ........ the NW variant's score (the maximum over the last row AND the last column) and its alignment's end
 *                           cell (the arg-max of one row) are different cells in the reference: "placed" has no single meaning
 *   band_width > 0 ........ banded scores -- unless valign_hip_set_band_placed(e, 1) asks for them, below
 *   traceback_policy = 1 .. the SSE/AVX tie-breaks
 *   score_width = 32, or a shape x scoring whose Smith-Waterman cells could leave int16 (the rule of the score path) --
 *                           unless valign_hip_set_placed_wide(e, 1) asks for them, below
 * "ran_placed" of valign_hip_describe says what the last call ran: "key" (register sweep, one end-cell key per lane), "rows"
 * (register sweep, a first-arg-max per row: more than 16 rows per lane, or scores too large for the key), "strip" (reads of
 * more than 1 024 rows or shapes no register geometry holds: the row strips' pointer-free forward pass), "chain" (band_placed,
 * below), "wide" (placed_wide, below), "none".                                                                               */
typedef struct {                     /* 12 bytes */
    int32_t score, read_end, ref_end;
} valign_hip_placed;

/* Placed scores under the band (key band_placed; flat API only).  0 (default): placed scores are refused with band_width > 0, as
 * ever.  1: with band_width > 0 valign_hip_score_placed_device / _host run the banded score sweep of the block chain with
 * end-cell tracking ("ran_placed": "chain") -- what a banded mapper asks: the banded score and where it ends, at a few tens of
 * percent over the sweep instead of a banded alignment.  With band_width == 0 the key is not read: the unbanded routes run as
 * before.  DEFINITION:
 *   band ........ the chain's block band, exactly as valign_hip_score_device computes it: row i has the inclusive column
 *                 window of its block on (B, A) = (16, 1), which valign_hip_describe reports after valign_hip_set_band_width
 *                 ("band_block_rows", "band_col_align"); every cell outside its row's window holds 0.
 *   score ....... the banded Smith-Waterman score of the pair as int32: valign_hip_score_device's value wherever that is
 *                 below 32767, where the short saturates -- the record does not.
 *   read_end, ref_end
 *                 (read_end - 1, ref_end - 1) is the first IN-BAND cell in row-major order that holds the maximum: the
 *                 earliest read row and, within it, the earliest reference column -- the rule of
 *                 src/Kernels/default/DefaultKernel.cpp:252-256 restricted to in-band cells.  0-based, half-open.
 *   empty ....... a pair whose banded maximum is 0 returns {0, 0, 0}.
 *   wide bands .. a band of at least 2 * max(R, F) gives exactly the unbanded placed records (where the chain plans a band
 *                 that wide: its rings must fit, below).
 *   read length . the route is the chain whatever the read length (banded scores already go there for short reads).
 * The chain runs on int32 cells whatever score_width says: score_width and the int16 range rule are not read on this route.
 * REFUSED under band_placed = 1 with a band: opt & 0xF == 1 and traceback_policy = 1, as above; a (shape, band, scoring) for
 * which the chain has no usable plan -- there is no fall-back to the row strips: their band is the (160, 4) one, a different
 * definition --; scores so large that the int32 cells ((R + F + 2) x |score| >= 2^28) or the end-cell key
 * ((min(R, F) x match + 1) << 4 beyond int32) could overflow.  tests/placed_band_ref.py restates the definition in numpy.
 * Other values than 0 / 1 are refused.                                                                                      */
int valign_hip_set_band_placed(valign_hip_engine *e, int on);

/* Placed and spanned scores on int32 cells (key placed_wide; flat API only).  0 (default): every call runs or is refused exactly
 * as above.  1: valign_hip_score_placed_device / _host and valign_hip_score_span_device / _host also accept the two kinds of
 * unbanded Smith-Waterman call the list above refuses for their cells -- calls with score_width = 32, and calls with
 * score_width = 0 whose shape x scoring could leave int16 (min(R, F) x match + 1 > 32000: 20 kbp x 20 kbp at match 2, 10 kbp x
 * 10 kbp at match 5) -- and runs them on a pointer-free int32 sweep of row strips ("ran_placed": "wide"): one int32 boundary
 * row per pair (two with affine gaps) and 8 bytes per pair of end cell between its launches, nothing else -- no pointer
 * stream, no walk.  DEFINITION: the record is the one defined above, unchanged --
 *   score ....... the Smith-Waterman maximum of the pair as int32.  The record does NOT saturate at 32767: it equals
 *                 valign_hip_score_device's value wherever that is below 32767 and valign_hip_aln.score of
 *                 valign_hip_align_cigar_device everywhere.
 *   read_end, ref_end
 *                 (read_end - 1, ref_end - 1) is the row-major first cell that holds the maximum
 *                 (src/Kernels/default/DefaultKernel.cpp:252-256); 0-based, half-open.
 *   empty ....... a pair whose maximum is 0 returns {0, 0, 0} (spanned: five zeros).
 *   spanned ..... the placed record plus the begin cell by the reversed-sweep rule below; the reverse sweep's engine of shape
 *                 (read_length, span_ref_length) carries the key and decides its own route.
 * WHAT THE KEY DOES NOT CHANGE: calls inside the int16 range with score_width 0 or 16 keep their routes ("key", "rows",
 * "strip") and kernels; score_width = 16 means "int16 or refuse" and stays refused, with the text above, on a shape x scoring
 * that can leave int16; opt & 0xF == 1, traceback_policy = 1 and band_width > 0 are refused (or run on the chain under
 * band_placed) as above -- the key is not read under a band.
 * REFUSED under placed_wide = 1: scores so large that the int32 cells could overflow, (R + F + 2) x |score| >= 2^28, with a
 * message that begins "placed_wide:".  Other values than 0 / 1 are refused.
 * "ran_placed" reads "wide" after such a call; "ran_span" joins the forward and the reverse route, so it may read "wide/wide",
 * "wide/key", ...; "placed_wide" of valign_hip_describe is the key and "placed_scratch_bytes" the boundary rows and end cells
 * the engine holds for the strip and wide routes.  Calls of one engine that take the route belong on one stream.            */
int valign_hip_set_placed_wide(valign_hip_engine *e, int on);

/* Device-resident: d_placed = n records.  Asynchronous on hip_stream, uses no pointer scratch and writes nothing but d_placed
 * (the strip path keeps its boundary rows and end cells in an engine-owned scratch: calls of one engine that take it belong
 * on one stream).                                                                                                            */
int valign_hip_score_placed_device(valign_hip_engine *e, int opt, long long n, const void *d_reads,
                                   const void *d_refs, void *d_placed, void *hip_stream);

/* Host pointers in, records out: the gather -> pinned staging -> H2D -> kernel -> D2H chunk pipeline of
 * valign_hip_score_host (4-bit classes under host_packing), 12 bytes per pair on the way back.                             */
int valign_hip_score_placed_host(valign_hip_engine *e, int opt, int n, const char *const *reads,
                                 const char *const *refs, valign_hip_placed *placed, int threads);

/* ---- spanned Smith-Waterman scores: begin and end cell without a traceback ----
 * A mapper reports where an alignment BEGINS (SAM's POS is ref_begin, the soft clip is read_begin).  Spanned scores give the
 * placed record plus the begin cell from TWO score sweeps: no pointer stream, no pointer scratch, no walk, no host round trip.
 * DEFINITION, for Smith-Waterman (opt & 0xF == 0), per pair:
 *   score, read_end, ref_end
 *                 exactly what valign_hip_score_placed_device returns for the pair.
 *   read_begin, ref_begin
 *                 Let P be the prefix rectangle read[0, read_end) x ref[0, ref_end).  The end cell is the first cell in row-major
 *                 order that holds the maximum, so it is the only cell of P that holds `score`, and every local alignment
 *                 inside P with that score ends in it.  Reverse both prefixes and run the same Smith-Waterman recurrence
 *                 (same scoring, same gap model, read steps and reference steps keeping their roles): that reversed matrix
 *                 has maximum `score`, in exactly the cells where an optimal alignment ending in the end cell can begin.
 *                 (read_begin, ref_begin) come from the FIRST cell in row-major order of the reversed matrix that holds
 *                 `score`: if that cell is (i', j'), 0-based, read_begin = read_end - 1 - i' and ref_begin = ref_end - 1 - j'.
 *                 In forward terms: of all optimal alignments that end in the end cell, the one that begins in the latest read
 *                 row and, within that row, the latest reference column.  0-based and half-open, as in valign_hip_aln.
 *   empty ....... a pair whose maximum is 0 returns five zeros.
 * GUARANTEED: the global alignment score of read[read_begin, read_end) against ref[ref_begin, ref_end) under the engine's
 * scoring equals `score`.
 * NOT GUARANTEED: equality with valign_hip_aln.read_begin / .ref_begin of valign_hip_align_cigar_device.  The walk follows the
 * fill's pointer tie-breaks; where two optimal alignments share the end cell it may begin elsewhere (on random pairs with the
 * CPU oracle's walk about one pair in 200 differed).  The two are not interchangeable.
 * The reverse sweep looks back span_ref_length = min(ref_length, read_length + (read_length x max(match, mismatch, 0) - 1) /
 * c) reference columns, c the cheapest price of one reference base against a gap in the read (|gap_read|; affine: min(|open_read|,
 * |ext_read|); c = 0: ref_length): no alignment of a positive score covers more, so the clipped sweep gives exactly the
 * unclipped records.  tests/span_ref.py restates the definition in numpy, unclipped.
 * REFUSED with a non-zero return and a message in valign_hip_last_error: everything valign_hip_score_placed_device refuses
 * without a band, with the same texts (opt & 0xF == 1, traceback_policy = 1, score_width = 32, a shape x scoring whose cells
 * could leave int16; the last two unless placed_wide = 1, above) -- and band_width > 0 WHATEVER band_placed says: the chain's block windows are not symmetric under
 * reversal, so a reversed banded sweep would be another band.  opt & 0xF > 1 does nothing, as everywhere.
 * "ran_span" of valign_hip_describe names the forward and the reverse route of the last call, joined ("key/key", "strip/strip",
 * ...; "none" before any, or when it was refused); "ran_placed" then reports the forward route; "span_ref_length" is the bound
 * above and "span_scratch_bytes" the scratch device-resident calls hold.                                                     */
typedef struct {                     /* 20 bytes */
    int32_t score, read_begin, read_end, ref_begin, ref_end;
} valign_hip_span;

/* Device-resident: d_spans = n records.  Asynchronous on hip_stream, no host synchronisation once the scratch exists.  The call
 * is cut into chunks so that the reversed prefixes and the two record buffers stay inside an engine-owned scratch of at most
 * 256 MiB (whole rounds of the forward sweep's waves); that scratch is reused chunk after chunk in stream order: calls of one
 * engine that use it belong on one stream.                                                                                   */
int valign_hip_score_span_device(valign_hip_engine *e, int opt, long long n, const void *d_reads,
                                 const void *d_refs, void *d_spans, void *hip_stream);

/* Host pointers in, records out: the chunk pipeline of valign_hip_score_placed_host (gather, 4-bit classes under
 * host_packing, H2D, kernels, D2H; small calls run on the pinned staging directly), 20 bytes per pair on the way back.       */
int valign_hip_score_span_host(valign_hip_engine *e, int opt, int n, const char *const *reads,
                               const char *const *refs, valign_hip_span *spans, int threads);

/* ---- spanned CIGARs: the alignment of the span, from the span's window instead of the full matrix ----
 * The fourth call of a mapper, after placed, spanned and suboptimal scores: the alignment itself.  valign_hip_align_cigar_device
 * fills and walks the whole read_length x ref_length matrix; after a spanned call the best local alignment is known to lie in
 * read[0, read_end) x ref[ref_end - span_ref_length, ref_end), so this call fills and walks THAT window -- pointer stream and fill
 * grow with span_ref_length (249 / 449 columns at 150 rows with linear 2 / -1 / -3 and affine -5 / -1 gaps), whatever ref_length is.
 * Results are valign_hip_aln records and `length << 4 | code` ops, as in the compact result format above.
 * DEFINITION, for Smith-Waterman (opt & 0xF == 0), per pair:
 *   coordinates . read_begin, read_end, ref_begin, ref_end are exactly the record valign_hip_score_span_device returns for the pair.
 *   ops ......... Take the alignment valign_hip_align_cigar_device would return for the pair (reversed read[0, read_end),
 *                 reversed ref[0, ref_end)) under the Default tie-breaks.  The ops are that alignment's columns read from last to
 *                 first, then classified and run-length encoded by vh_cigar's column rule (above).  Read backwards, that
 *                 alignment is one of read[read_begin, read_end) against ref[ref_begin, ref_end): its end cell is the spanned
 *                 record's begin cell (both are the first cell in row-major order of the reversed matrix that holds `score`),
 *                 and its walk ends in the reversed origin, because the forward end cell is the only cell of the prefix
 *                 rectangle that holds `score`.  The reversed reference is clipped to span_ref_length columns: no cell beyond
 *                 the clip can hold `score`, and the pointers inside the clip do not depend on later columns.
 *   score ....... the returned alignment re-scored, as in valign_hip_aln.
 *   empty ....... a pair whose maximum is 0 returns an all-zero record and no ops.
 * GUARANTEED: `score` equals the placed score of the pair (valign_hip_score_placed_device), and the ops consume exactly
 * read_end - read_begin read bases and ref_end - ref_begin reference bases.  (For sequences that hold no '-' byte: the column
 * rule reads a literal '-' as a gap, as vh_cigar does, and the begin coordinates -- the ends minus the non-gap bases of the
 * rows, as in valign_hip_aln -- and the re-score then follow the ops.)
 * NOT GUARANTEED: equality of the ops (or of read_begin / ref_begin) with those of valign_hip_align_cigar_device on the forward
 * pair.  Both are optimal alignments that end in the same cell, walked under tie-breaks in opposite directions; where two
 * optimal alignments share the end cell they may differ.  The two are not interchangeable.
 * REFUSED with a non-zero return and a message in valign_hip_last_error: everything valign_hip_score_span_device refuses, with
 * the same texts (opt & 0xF == 1; traceback_policy = 1; every band_width > 0, whatever band_placed says; score_width = 32 or a
 * shape x scoring whose cells could leave int16, unless placed_wide = 1) -- and whatever the alignment route of the window's
 * shape refuses, prefixed with "spanned CIGARs: ".  extended must be 0 or 1; anything else is refused.
 * NOT REFUSED: under placed_wide = 1 the forward sweep runs on int32 cells and the window's alignment picks its own cells, as
 * valign_hip_align_device always does.  pointer_scratch_cap_mb and trace_checkpoints apply to the window's alignment.
 * opt & 0xF > 1 does nothing, as everywhere.
 * "ran_span_cigar" of valign_hip_describe names the forward route and the window's "ran_align_fill", joined ("key/tag_prof_key",
 * "strip/strip_ckpt", ...; "none" before any call, or when it was refused); "ran_result_format" is then "cigar" and
 * "span_cigar_scratch_bytes" the scratch the calls hold.                                                                       */

/* Device-resident: asynchronous on hip_stream.  d_recs = n records, d_ops = n * ops_stride uint32: a pair stores its first
 * min(n_ops, ops_stride) ops in reading order at d_ops + pair * ops_stride, words past them are not written, and n_ops always
 * says how many there are.  The call is cut into chunks (whole rounds of the forward sweep's waves) so that the reversed
 * prefixes, the forward records and the window's rows -- 3 * (read_length + span_ref_length) + 20 bytes per pair -- stay inside
 * an engine-owned scratch of at most 768 MiB, reused chunk after chunk in stream order: calls of one engine that use it belong
 * on one stream.                                                                                                             */
int valign_hip_align_span_device(valign_hip_engine *e, int opt, long long n, const void *d_reads,
                                 const void *d_refs, int extended, void *d_recs, void *d_ops,
                                 int ops_stride, void *hip_stream);

/* Host pointers in, packed results out, with the contract of valign_hip_align_cigar_host: recs[n], offsets[n + 1] (offsets[0] =
 * 0), pair p's ops are ops[offsets[p] .. offsets[p + 1]); if the call needs more than ops_cap ops it returns non-zero,
 * *ops_needed holds the total and recs / offsets are complete; n = 0 sets offsets[0] = 0; opt & 0xF > 1 writes nothing.  Per
 * chunk: gather, H2D, the launches above with a records-only sink, a scan of n_ops, the ops packed at their offsets beside the
 * records and ONE copy back -- 24 bytes per pair, 4 per op and 8 per chunk ("cigar_d2h_bytes"); the rows never cross PCIe.
 * Chunks follow one another on one stream and do not overlap.                                                               */
int valign_hip_align_span_host(valign_hip_engine *e, int opt, int n, const char *const *reads,
                               const char *const *refs, int extended, valign_hip_aln *recs,
                               uint32_t *ops, long long ops_cap, long long *offsets,
                               long long *ops_needed, int threads);

/* ---- suboptimal Smith-Waterman scores: runner-up score and column without a traceback ----
 * A mapper computes mapping quality from the SECOND-best local alignment score: SSW's score2 / ref_end2, BWA's sub -- the best
 * score that ends at least `mask` reference columns away from where the best alignment ends.  Suboptimal scores give the placed
 * record plus that pair of numbers from the ONE placed sweep: no second sweep, no DP matrix, no host round trip.
 * DEFINITION, for Smith-Waterman (opt & 0xF == 0), per pair, with the caller's mask >= 0 per call:
 *   score, read_end, ref_end
 *                 exactly what valign_hip_score_placed_device returns for the pair.
 *   trimmed lengths
 *                 Rp is 1 + the position of the last ACGT byte (either case) of the read row, 0 if there is none; Fp the same
 *                 for the reference row: the lengths without trailing non-ACGT bytes that ragged batching uses.
 *   colmax[j] ... for 0 <= j < Fp, the maximum of H[i][j] over 0 <= i < Rp, H the Smith-Waterman matrix of the pair (interior
 *                 non-ACGT bytes score 0 as everywhere).
 *   candidates .. the columns j with |j - (ref_end - 1)| > mask.
 *   score2 ...... the largest colmax[j] over the candidates.
 *   ref_end2 .... ref_end2 - 1 is the SMALLEST candidate column that holds score2.  Both are 0 where there is no candidate or the
 *                 largest is 0.
 *   empty ....... a pair whose score is 0 returns five zeros.
 * Rows and columns beyond the trimmed lengths are not candidates: a non-ACGT byte scores 0 against anything, so a value runs
 * down the diagonal through padding unchanged, and a padded read would report its own best score again as the runner-up.
 * THE CALLER PICKS THE MASK: columns before the window hold the best alignment's own partial scores (the prefixes of the best
 * alignment end there), so a mask that is too small reports those.  SSW uses half the read length.
 * REFUSED with a non-zero return and a message in valign_hip_last_error: mask < 0; everything unbanded placed scores refuse,
 * with the same texts (opt & 0xF == 1, traceback_policy = 1, score_width = 32, a shape x scoring whose cells could leave int16)
 * -- placed_wide = 1 does not open the int32 sweep here; every band_width > 0, WHATEVER band_placed says; and the shapes placed
 * scores send to the row strips (reads of more than 1024 rows, or no register geometry).  The sweep holds 1 KiB of LDS per
 * wave more than the placed one (the column ring): a block whose rings no longer fit runs with half as many waves, and only
 * where ONE wave's reference tables come within 1 KiB of the 160 KiB -- a forced geometry on a very long reference, such as
 * 16 x 10 at 16,200 columns; unforced calls take the row strips long before -- the call is refused too ("... leave no room for
 * its column ring in the LDS").  opt & 0xF > 1 does nothing, as everywhere.
 * "ran_subopt" of valign_hip_describe is the track of the last call's sweep, key or rows ("none" before any, or when it was
 * refused); "subopt_scratch_bytes" the scratch device-resident calls hold; "subopt_ring_cols" the columns a lane group of that
 * sweep gathers in LDS before the wave writes them out.  tests/subopt_ref.py restates the definition in numpy.              */
typedef struct {                     /* 20 bytes */
    int32_t score, read_end, ref_end, score2, ref_end2;
} valign_hip_subopt;

/* Device-resident: d_subopt = n records.  Asynchronous on hip_stream, no host synchronisation once the scratch exists.  The call
 * is cut into chunks of whole rounds of the sweep's waves (of whole waves where a round is larger) so that the column maxima (4 bytes per column and pair of pairs) stay
 * inside an engine-owned scratch of at most 256 MiB; that scratch is reused chunk after chunk in stream order: calls of one
 * engine that use it belong on one stream.                                                                                   */
int valign_hip_score_subopt_device(valign_hip_engine *e, int opt, long long n, const void *d_reads,
                                   const void *d_refs, int mask, void *d_subopt, void *hip_stream);

/* Host pointers in, records out: the chunk pipeline of valign_hip_score_placed_host, 20 bytes per pair on the way back.      */
int valign_hip_score_subopt_host(valign_hip_engine *e, int opt, int n, const char *const *reads,
                                 const char *const *refs, int mask, valign_hip_subopt *subopt, int threads);

/* ---- extension scores: anchored score, end cell and read-end score per pair, without a traceback ----
 * Every call above is Smith-Waterman: a free start anywhere in the matrix.  A seed-and-extend mapper (BWA-MEM's ksw_extend,
 * minimap2's extension stage) has an ANCHOR -- a seed that fixes where read and reference correspond -- and asks, from there:
 * what is the best score of an alignment that starts exactly at the anchor and ends anywhere, and where does it end; and what is
 * the best score if the read is consumed to its last base (end-to-end or clip?).  Extension scores answer both from one sweep.
 * DEFINITION, for opt & 0xF == 0, per pair; the engine's scoring applies, with the usual class rule: `match` or `mismatch`
 * between two ACGT bases of either case, 0 for any other pair of bytes, interior ones included.
 *   anchor ...... the alignment starts before read[0] and ref[0]: THE CALLER PASSES THE SEQUENCE AFTER ITS SEED.  For a leftward
 *                 extension the caller reverses both sequences.
 *   trimmed lengths
 *                 Rp is 1 + the position of the last ACGT byte (either case) of the read row, 0 if there is none; Fp the same
 *                 for the reference row: the rule of the suboptimal scores and of ragged batching.
 *   matrix ...... X(-1,-1) = 0.  The border column X(i,-1) is a gap of i + 1 read bases against nothing: (i + 1) * gap_ref with
 *                 linear gaps, open_ref + i * ext_ref with affine gaps.  The border row X(-1,j) is the same in the other
 *                 direction: (j + 1) * gap_read, or open_read + j * ext_read.  Inside, the library's linear or Gotoh recurrence
 *                 with NO FLOOR AT ZERO: X(i,j) is the best score of any DIAG / UP / LEFT path from the origin to the cell,
 *                 maximal gap runs priced open + (k - 1) * ext per direction.
 *   score ....... max(0, max X(i,j)) over 0 <= i < Rp, 0 <= j < Fp.
 *   read_end, ref_end
 *                 (read_end - 1, ref_end - 1) is the row-major first cell that holds score (DefaultKernel.cpp:252-256); half-open,
 *                 0-based ends.
 *   empty ....... if score is 0, then score = read_end = ref_end = 0.
 *   gscore ...... the maximum of X(Rp - 1, j) over the candidates -1 <= j < Fp; the border column counts as j = -1.  int32, may
 *                 be negative.
 *   gref_end .... gref_end - 1 is the smallest candidate column that holds gscore (0: the border column).
 *   Rp = 0 ...... the record is five zeros.
 * Columns at or beyond Fp are not candidates for gscore: padding scores 0 against anything, and a read longer than the trimmed
 * reference would otherwise ride its tail down the padding for free.
 * NOT BUILT: Z-drop or X-drop termination -- every cell is swept.  An end bonus is not part of the scores -- the caller compares
 * gscore + bonus with score itself; extension alignments (valign_hip_align_extend_*, below) take it as the rule that picks the end
 * cell they walk from.  ragged_batching and half_float_cells are not read.
 * REFUSED with a non-zero return, a message in valign_hip_last_error and "ran_extend": "none": opt & 0xF == 1;
 * traceback_policy = 1; band_width > 0, WHATEVER band_placed says; score_width = 32, WHATEVER placed_wide says; a shape x
 * scoring whose cells could leave int16 -- signed cells: min(R, F) * max(match, mismatch, 0) above 32000, or the all-gaps path
 * to the far corner (R reference-direction steps and F read-direction steps at their worst price) plus the largest single addend
 * below -32000; and the shapes placed scores send to the row strips (reads of more than 1024 rows, or no register geometry).
 * The last three -- score_width = 32, the int16 range under score_width = 0, the row strips' shapes -- run on int32 cells under
 * valign_hip_set_extend_wide(e, 1), below.  opt & 0xF > 1 does nothing, as everywhere.
 * "ran_extend" of valign_hip_describe is "rows" after a call that ran on the register sweep, "wide" (extend_wide, below) after
 * one that ran on the int32 sweep ("none" before any, or when it was refused).  The register sweep's device call holds no
 * scratch.  tests/extend_ref.py restates the definition in numpy.                                                          */
typedef struct {                     /* 20 bytes */
    int32_t score, read_end, ref_end, gscore, gref_end;
} valign_hip_extend;

/* Device-resident: d_extend = n records.  Asynchronous on hip_stream, no host synchronisation: one launch, nothing but the
 * records is written.                                                                                                        */
int valign_hip_score_extend_device(valign_hip_engine *e, int opt, long long n, const void *d_reads,
                                   const void *d_refs, void *d_extend, void *hip_stream);

/* Host pointers in, records out: the chunk pipeline of valign_hip_score_placed_host, 20 bytes per pair on the way back.      */
int valign_hip_score_extend_host(valign_hip_engine *e, int opt, int n, const char *const *reads,
                                 const char *const *refs, valign_hip_extend *extend, int threads);

/* Extension scores on int32 cells and row strips (key extend_wide; flat API only).  0 (default): every extension call runs or is
 * refused exactly as stated above.  1: a call that would be refused for one of THREE reasons runs instead, with the same
 * definition and the same record, on the int32 extension sweep (score_extend_wide_kernel: signed int32 cells, 512-row strips, a
 * launch per strip, boundary rows handed from strip to strip; "ran_extend": "wide", "ran_extend_geometry": "none"):
 *   - score_width = 32;
 *   - a shape x scoring whose cells could leave int16, under score_width = 0 (16 means "int16 or refuse" and stays refused);
 *   - reads of more than 1024 rows, and shapes without a register geometry -- whatever score_width says: the long reads a
 *     seed-and-extend mapper extends on.
 * Every other call decides as with 0: a call the register sweep serves keeps it ("rows"), and opt & 0xF == 1,
 * traceback_policy = 1 and every band_width > 0 stay refused with their texts.  placed_wide is not read by extension calls, nor
 * extend_wide by placed, spanned or suboptimal ones.  Values and coordinates are int32 from the cell to the record: nothing
 * saturates (33 x 1000 is 33000).
 * REFUSED under extend_wide = 1, with a message that begins "extend_wide:": a shape x scoring whose cells could leave +-2^28 --
 * min(R, F) * max(match, mismatch, 0) above 2^28, or the all-gaps path to the far corner plus the largest single addend below
 * -2^28 (the bounds of the int16 rule, at this width).  The gap states of the two borders are a finite value of -2^29 that
 * drifts down by an extension per step: the bound keeps it below every cell and inside int32.  Other values than 0 / 1 are
 * refused.
 * The device call is cut into chunks whose boundary rows fit the engine's strip scratch (the placed int32 sweep's, shared with
 * it: calls of one engine that use it belong on one stream); per pair it also holds a 20-byte partial record and the two trimmed
 * lengths.  The host call is the chunk pipeline with the strip path's chunk sizes, on one stream.
 * KNOWN: a short read fills a fraction of its one 512-row strip, as on the placed int32 sweep -- the register sweep is the route
 * for short reads wherever the rule lets it run.  Z-drop and a band around the anchor's diagonal remain unbuilt; extension
 * alignments (below) refuse the calls this key moves to the int32 sweep.
 * "extend_wide" of valign_hip_describe is the key.                                                                           */
int valign_hip_set_extend_wide(valign_hip_engine *e, int on);

/* Banded extension scores: a band on the ANCHOR's diagonal (key extend_band; flat API only).  The sentence above that calls a
 * band around the anchor's diagonal unbuilt is qualified here: under this key the band is built, for the extension SCORES.
 * Seed-and-extend callers (ksw_extend, ksw_extz) extend inside a band around the diagonal i = j of their anchor; the other band
 * entry points (band_width alone, band_placed, band_nw) are Smith-Waterman or NW matrices on the scaled diagonal i * F / R.
 *   0 (default): nothing changes -- band_width > 0 refuses extension calls with the text stated above.
 *   1 with band_width > 0: valign_hip_score_extend_device / _host run BANDED on the int32 strip sweep (the BANDED instances of
 *     score_extend_wide_kernel), whatever the read length, score_width (0 or 32) or extend_wide say; "ran_extend": "band",
 *     "ran_extend_geometry": "none".  With band_width == 0 the key is not read.  Placed, spanned, suboptimal and alignment calls
 *     never read it.  Other values than 0 / 1 are refused.
 * DEFINITION.  The record, the trimmed lengths Rp / Fp, the matrix X, the recurrence and the tie rules are exactly those of the
 * extension scores, above.  The only difference is that some cells are ABSENT.
 *   w ........... band_width / 2, the library's "diagonals" convention; band_width = 1 gives w = 0.
 *   blocks ...... rows are taken in blocks of B = VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS = 8 consecutive read positions counted from
 *                 row 0: block b holds rows [8b, 8b + 8) -- one lane's rows on the sweep.
 *   present ..... cell (i, j) with 0 <= i < R and -1 <= j < F is present iff 8*(i/8) - w <= j <= 8*(i/8) + 7 + w.  The border
 *                 column j = -1 counts like any other column.
 *   border row .. cell (-1, j) is present iff j + 1 <= w.  (-1, -1) is always present.
 *   absent ...... an absent cell is never a candidate of a neighbour, a maximum or an arg-max.  With affine gaps H, E and F are
 *                 all absent.
 *   borders ..... present border cells hold the unbanded closed-form values.  Every present cell has a present path from the
 *                 origin, so the closed forms stay valid.
 *   per-cell band With B = 1 this is the per-cell band |i - j| <= w.  The library computes the B = 8 superset: more cells mean
 *                 more paths, so for score and gscore: per-cell band <= result <= unbanded.
 *   limit ....... a band with w >= max(R, F) gives exactly the unbanded record.
 *   score, read_end, ref_end
 *                 as defined above, taken over the present cells with i < Rp and j < Fp.
 *   gscore, gref_end
 *                 taken over the present candidates -1 <= j < Fp of row Rp - 1.
 *   unreached ... if no candidate is present (8*((Rp-1)/8) - w > Fp - 1), the read end is unreached: gscore =
 *                 VALIGN_HIP_EXTEND_UNREACHED (INT32_MIN) and gref_end = 0.  Rp = 0 is still five zeros.
 * REFUSED under extend_band = 1 with band_width > 0, "ran_extend": "none": opt & 0xF == 1 and traceback_policy = 1, with the
 * texts stated above; score_width = 16 ("int16 or refuse"), with a text that begins "extend_band:"; a shape x scoring that
 * fails the band's int32 bound, with another text that begins "extend_band:" -- under a band the path "down the border column,
 * then along the row" may be absent, so the bottom of the cell range is R down steps, F right steps and min(R, F) diagonal steps,
 * each at its worst price, plus the largest single addend, which must stay above -2^28; the top bound and the sentinel's
 * conditions are those of extend_wide.  Extension alignments (valign_hip_align_extend_*) under band_width > 0 are refused with a
 * text that starts "extension alignments: not built under a band" (key off: the text stated above).
 * The scratch, the chunks and the one-stream host path are those of extend_wide.
 * KNOWN: the band runs on the strip sweep only.  Short reads under a band fill a fraction of their one 512-row strip and are slower
 * than the unbanded int16 register sweep, which has no banded form; there is no sub-wave geometry for them.  Z-drop, and extension
 * alignments under a band or on int32 cells, remain unbuilt.
 * "extend_band" of valign_hip_describe is the key, "extend_band_block_rows" is B.  tests/extend_band_ref.py restates the definition
 * in numpy.                                                                                                                   */
#define VALIGN_HIP_EXTEND_BAND_BLOCK_ROWS 8
#define VALIGN_HIP_EXTEND_UNREACHED (-2147483647 - 1)
int valign_hip_set_extend_band(valign_hip_engine *e, int on);

/* ---- extension alignments: the CIGAR of an extension, from the anchor to the chosen end cell ----
 * Extension scores say how far to extend and whether to go end-to-end or clip; this call returns the alignment of that extension.
 * No other alignment call can: Smith-Waterman has a free start and a floor at zero, the NW variant a free row 0, spanned CIGARs
 * place a local alignment.  Here both borders are gap-priced, the path is forced through the anchor, and the walk runs from a
 * given end cell back to (-1, -1).
 * DEFINITION, for opt & 0xF == 0, per pair, with X, Rp, Fp, score, read_end, ref_end, gscore and gref_end exactly as the
 * extension scores define them (above):
 *   end cell .... end_bonus < 0: the best cell (read_end - 1, ref_end - 1).  end_bonus >= 0: the read end (Rp - 1, gref_end - 1)
 *                 if Rp > 0 and (int64) gscore + end_bonus >= score, otherwise the best cell; the column may be the border
 *                 column -1.  |gscore| <= 32000 on this route, so end_bonus = INT32_MAX means "always the read end".  Ties go to
 *                 the read end.
 *   empty ....... the best cell was chosen and score == 0, or Rp == 0: an all-zero record and no ops.
 *   walk ........ from the end cell back to (-1, -1), decided on cell values.  Linear gaps, at an interior cell: DIAG if
 *                 X(i,j) == X(i-1,j-1) + S(i,j), else UP if X(i,j) == X(i-1,j) + gap_ref, else LEFT (the Default priority).
 *                 Affine gaps: the library's three-state rule -- at H: DIAG if h == diag, else the vertical state if h == f, else
 *                 the horizontal state; inside a gap state: emit one column, then stay in the state iff its value differs from
 *                 its "open" candidate (f != f_open, e != e_open), otherwise return to H.  On a border cell the walk is at H and
 *                 follows the border: UP on column -1, LEFT on row -1 (the gap states do not exist on the borders: a gap run that
 *                 turns the corner opens again).  It stops at (-1, -1).
 *   ops ......... the columns in reading order, classified and run-length encoded by the column rule of valign_hip_align_cigar_*
 *                 (extended: 0 = M, 1 = '=' / X), length << 4 | code.  A first op of I or D is legal: a gap directly after the seed.
 *   record ...... read_begin = ref_begin = 0; read_end, ref_end: the end cell + 1 (ref_end = 0 for the border column); score: the
 *                 ops re-scored under the engine's scoring, as in valign_hip_aln.
 * GUARANTEED: score == X(end cell) -- the extension record's score, or its gscore, whichever end was chosen -- and the ops
 * consume exactly read_end read bases and ref_end reference bases; for sequences without a literal '-' byte (the caveat of spanned
 * CIGARs).
 * Records, ops, ops_stride, n_ops on overflow, offsets, ops_cap, ops_needed, n = 0 and opt & 0xF > 1 follow the contracts of
 * valign_hip_align_cigar_device / _host exactly.  If d_extend / extend is not null it receives the pair's valign_hip_extend
 * record, bit for bit what valign_hip_score_extend_device returns.
 * REFUSED with a non-zero return, a message in valign_hip_last_error and "ran_extend_align": "none": everything
 * valign_hip_score_extend_device refuses with extend_wide = 0, with the same texts; under extend_wide = 1, any call whose
 * extension route is "wide", with a text that begins "extension alignments:" (the int32 / row-strip form keeps no back
 * pointers); extended not 0 or 1; ops_stride < 1; null result buffers.
 * NOT BUILT: Z-drop / X-drop, a band around the anchor's diagonal, the int32 route.  ragged_batching and half_float_cells are not
 * read.
 * The device call is asynchronous on hip_stream.  It is cut into chunks that keep the pointer stream (2 bits per cell, twice that
 * with affine gaps) under pointer_scratch_cap_mb and the walk's rows under the compact format's rows scratch; the chunks reuse both
 * in stream order, and both are shared with the other alignment calls: calls of one engine belong on one stream.
 * "ran_extend_align" of valign_hip_describe is "rows" after a call that ran ("none" before any, or when it was refused),
 * "ran_extend_align_geometry" the geometry whose fill ran, "align_ptr_bytes_per_pair" the pointer-stream bytes a pair holds in that
 * fill (after a call that ran), "extend_align_scratch_bytes" the pointer scratch, end cells and staged extension records the engine
 * holds.  tests/extend_align_ref.py restates the definition in numpy.                                                          */
int valign_hip_align_extend_device(valign_hip_engine *e, int opt, long long n, const void *d_reads, const void *d_refs,
                                   int end_bonus, int extended, void *d_recs, void *d_ops, int ops_stride,
                                   void *d_extend /* may be null */, void *hip_stream);

/* Host pointers in, packed results out: chunk after chunk -- gather, H2D, fill, walk, the count pass, the scan, the emit pass and
 * ONE copy of records, extension records (where asked for) and ops back.                                                      */
int valign_hip_align_extend_host(valign_hip_engine *e, int opt, int n, const char *const *reads, const char *const *refs,
                                 int end_bonus, int extended, valign_hip_aln *recs, uint32_t *ops, long long ops_cap,
                                 long long *offsets, long long *ops_needed, valign_hip_extend *extend /* may be null */, int threads);

/* Banded extension alignments: CIGARs inside the anchor's band (key extend_band_align; flat API only).  The sentences above that
 * call extension alignments under a band, or on int32 cells, unbuilt or refused are qualified here: under this key they are built,
 * on the banded int32 strip sweep, as the extend_band section qualified the sentence before it.
 *   0 (default): every call runs or is refused exactly as stated above, with the texts stated above.
 *   1 with band_width > 0 and extend_band = 1: valign_hip_align_extend_device / _host run BANDED (align_extend_band_fill_kernel:
 *     the BANDED extension sweep that also streams a back pointer per present cell; a launch per 512-row strip), whatever the read
 *     length, score_width (0 or 32) or extend_wide say; "ran_extend_align": "band", "ran_extend_align_geometry": "none".  With
 *     band_width == 0 or extend_band == 0 the key is not read: the register route and the refusals above stand.  No other call
 *     reads the key.  Other values than 0 / 1 are refused with "extend_band_align must be 0 or 1".
 * DEFINITION.
 *   matrix ...... X, E, G, the trimmed lengths Rp / Fp, w = band_width / 2, the blocks of B = 8 rows, present and absent cells and
 *                 the present border cells with their closed forms are exactly those of banded extension scores, above.
 *   extension record
 *                 the banded one, bit for bit what valign_hip_score_extend_device returns under the same keys -- gscore =
 *                 VALIGN_HIP_EXTEND_UNREACHED, gref_end = 0 for an unreached read end included.
 *   end cell .... the rule of extension alignments, computed in 64 bits.  An unreached read end is never chosen, whatever end_bonus
 *                 is: INT32_MIN + INT32_MAX = -1 < 0 <= score, so the rule already says so.  end_bonus = INT32_MAX still means
 *                 "the read end wherever it is reached": |gscore| < 2^28 on this route.
 *   empty ....... the best cell was chosen and score == 0, or Rp == 0.
 *   walk ........ the rules of extension alignments, on cell values; an absent candidate equals nothing.  (i, -1) present implies
 *                 (i-1, -1) present, (-1, j) present implies (-1, j-1) present, and every present interior cell has a present
 *                 candidate: the walk never leaves the band.
 * GUARANTEED: score == X_band(end cell), and the ops consume exactly read_end read bases and ref_end reference bases; the
 * literal-'-' caveat applies as elsewhere.
 *   limit ....... w >= max(R, F) gives the unbanded extension alignment: on a call the register sweep serves, its result; on a call
 *                 it refuses (int32 cells, long reads), the definition as tests/extend_align_ref.py restates it.
 * Records, ops, ops_stride, overflow, offsets, ops_cap / ops_needed, n = 0, opt & 0xF > 1 and d_extend follow
 * valign_hip_align_extend_* exactly.
 * REFUSED under the key, with "ran_extend_align": "none": opt & 0xF == 1 and traceback_policy = 1, with their texts;
 * score_width = 16, with the text that begins "extend_band:"; a shape x scoring that fails the band's int32 bound, with its
 * "extend_band:" text; extended not 0 or 1; ops_stride < 1; null result buffers.
 * NOT BUILT, still: Z-drop / X-drop; a register (int16, sub-wave) form of the band -- short reads under a band fill a fraction of
 * one 512-row strip, as for the scores; checkpointed pointers for this route.
 * The pointer stream holds 2 bits per swept step and row (twice that with affine gaps) of every strip's window, in the layout of
 * versalignlib_amd/csrc/extend_band_align_plan.h; chunks keep it under pointer_scratch_cap_mb, the boundary rows in the strip
 * scratch banded extension scores use and the walk's rows in the compact format's rows scratch.  Calls of one engine belong on one
 * stream.
 * valign_hip_describe: "extend_band_align" is the key; after such a call "ran_extend_align" is "band" and
 * "ran_extend_align_geometry" "none", "align_ptr_bytes_per_pair" the band's pointer bytes per pair, "extend_align_scratch_bytes" the
 * pointer scratch, end cells and staged extension records the engine holds, "ran_extend_align_chunks" the chunks the call was cut
 * into.  tests/extend_band_align_ref.py restates the definition in numpy.                                                      */
int valign_hip_set_extend_band_align(valign_hip_engine *e, int on);

/* Extension Z-drop: rows stop counting at the first row that drops (key extend_zdrop; flat API only).  The three sentences above
 * that say "NOT BUILT: Z-drop" are qualified here: under this key a row-wise Z-drop is built, on the int32 strip sweep, as the
 * extend_band section qualified the sentence before it.  X-drop stays unbuilt.
 *   Z = 0 (default): every call runs or is refused exactly as stated above.
 *   0 < Z <= 2^30: valign_hip_score_extend_* and valign_hip_align_extend_* apply the rule below.  Only these calls read the key.
 *     Values outside [0, 2^30] are refused with "extend_zdrop must be in [0, 2^30]".
 * DEFINITION.  The matrix X, the trimmed lengths Rp / Fp, the recurrence and the tie rules are exactly those of extension scores;
 * under extend_band = 1 with band_width > 0 the present cells are those of banded extension scores.  No cell value changes: only
 * which rows count changes.
 *   row maxima ... for row i, 0 <= i < Rp, m_i is the maximum of X(i, j) over the present candidates -1 <= j < Fp -- the border
 *                  column counts -- and c_i the smallest such column.  A row with no present candidate is skipped: it neither
 *                  updates anything nor drops (under a band such rows are a suffix).
 *   running best . (M, Mi, Mj) starts at the anchor (0, -1, -1).  Rows are taken in order.  m_i > M: (M, Mi, Mj) = (m_i, i, c_i).
 *                  Otherwise, with di = i - Mi and dj = c_i - Mj, pen = (di - dj) * |ext_ref| if di > dj, else (dj - di) *
 *                  |ext_read| (linear gaps: |gap_ref|, |gap_read|), and the row DROPS iff M - m_i - pen > Z.
 *   drop row ..... T is the first dropping row, Rp if none drops.
 *   record ....... score = M, read_end = Mi + 1, ref_end = Mj + 1 as they stand at T -- three zeros when M = 0.  This is the
 *                  row-major first maximum over the rows < T, because border values are never positive.  T == Rp: gscore / gref_end
 *                  as without the key, the band's unreached closed form included.  T < Rp: the read end is unreached, gscore =
 *                  VALIGN_HIP_EXTEND_UNREACHED and gref_end = 0.  Rp = 0 is five zeros.
 *   alignments ... the extension record is the one above; the end-bonus rule then never picks the read end of a dropped pair (as for
 *                  the band's unreached read end), and the alignment is that of the pair cut to its first T rows.
 *   limits ....... Z >= 2^29 never drops and gives the record of Z = 0 bit for bit.  Nothing overflows on int32 cells: within
 *                  extend_int32_ok / extend_band_int32_ok every cell lies in [-2^28, 2^28], so 0 <= M - m_i <= 2^29; |di - dj| <= R + F
 *                  <= 32767 and a price is at most 32768, so 0 <= pen < 2^30; M - m_i - pen lies in (-2^30, 2^29] and Z <= 2^30.
 * This follows BWA's ksw_extend rule with this library's rows as read positions.  There is no floor at zero and the row range does
 * not shrink as ksw_extend's does; parity with BWA's numbers is not claimed.
 * ROUTES under Z > 0 (versalignlib_amd/csrc/extend_zdrop.h: extend_zdrop_choice, extend_zdrop_align_choice).  opt & 0xF == 1 and
 * traceback_policy = 1 are refused first, with their texts.
 *   scores, band_width > 0: as without the key -- "band" under extend_band = 1, with its refusals; the band's refusal without it.
 *   scores, band_width == 0: the int32 strip sweep ("ran_extend": "wide") whatever extend_wide, the read length and score_width 0 /
 *     32 say; refused with texts that begin "extend_zdrop:" for score_width = 16 and where the int32 bound of extend_wide fails.
 *     KNOWN: the int16 register sweep has no Z-drop form, so a 150-row read under the key fills 150 of its strip's 512 rows.
 *   alignments: only on the banded route (band_width > 0, extend_band = 1, extend_band_align = 1); every other call is refused with
 *     one "extend_zdrop:" text, which says that a band of 2 * max(read_length, ref_length) is the unbanded alignment.
 * COST.  A wave sweeps two pairs, a launch 512 rows of every pair.  A strip below the drop rows of both pairs of a wave returns
 * before its set-up; a strip that holds a drop row still runs to its end (no in-strip stop).
 * NOT BUILT: a Z-drop form of the int16 register sweep; an in-strip stop; an anti-diagonal (ksw_extz-style) rule, which a
 * strip-after-strip sweep cannot evaluate in order; X-drop.
 * valign_hip_describe: "extend_zdrop" is the key; "ran_extend_zdrop" the Z the last extension call ran under, or 0;
 * "extend_zdrop_skipped_waves" the waves that skipped a strip in the last such call (of a host call: in its last chunk).
 * "ran_extend" / "ran_extend_align" keep "wide" / "band".  tests/extend_zdrop_ref.py restates the definition in numpy.          */
int valign_hip_set_extend_zdrop(valign_hip_engine *e, int Z);

/* Extension Z-drop on the int16 register sweep (key extend_zdrop_rows; flat API only).  The sentences of the section above that say
 * "KNOWN: the int16 register sweep has no Z-drop form" and "NOT BUILT: a Z-drop form of the int16 register sweep" are qualified
 * here: under this key that form is built, for scores and for unbanded alignments.  The rule, the record and the limits are those
 * of extend_zdrop, word for word; only where the call runs changes.
 *   on = 0 (default): every call runs or is refused exactly as stated above, "ran_extend": "wide" for unbanded calls under Z > 0 and
 *     both "extend_zdrop:" texts included.
 *   on = 1: read by valign_hip_score_extend_* and valign_hip_align_extend_* only, and only where extend_zdrop > 0 and band_width == 0.
 *     Z = 0 under the key is the call without either key.  Other values are refused with "extend_zdrop_rows must be 0 or 1".
 * ROUTES under on = 1, Z > 0, band_width == 0 (versalignlib_amd/csrc/extend_zdrop.h: extend_zdrop_rows_choice,
 * extend_zdrop_rows_align_choice).  opt & 0xF == 1 and traceback_policy = 1 are refused first, with their texts.
 *   scores: where the call without extend_zdrop runs the register sweep it runs there ("ran_extend": "rows"), score_width = 16
 *     included; everything else answers as under extend_zdrop alone -- "wide", or its refusals: score_width = 32, cells that leave
 *     int16 and reads of more than 1,024 rows run "wide".
 *   alignments: where the call without extend_zdrop runs the register sweep it runs there ("ran_extend_align": "rows"): unbanded
 *     Z-dropped extension alignments.  Every other unbanded call is refused with one "extend_zdrop:" text, which says that the int32
 *     route of unbanded extension alignments has no Z-drop form.  The banded route answers as above.
 * HOW.  The register sweep ends with every row's maximum and first column in registers, so the drop row is decided after the last
 * step: each lane combines its rows, an exclusive prefix arg-max runs over the lanes of the pair's group, each lane replays its rows
 * from its prefix, and T is the smallest row any lane answers (extend_zdrop.h states why that is the serial rule's T).  No cell, no
 * back pointer and no step of the sweep changes; every cell is still swept (no in-sweep stop).  An alignment's walk starts in the
 * best cell before T, from where it only moves up and left; the read end is picked only where nothing dropped.
 *   limits ....... the register route runs only where every cell stays inside int16, so 0 <= M - m_i <= 65535; 0 <= pen < 2^30 as
 *                  above; M - m_i - pen lies in (-2^30, 2^16) and Z <= 2^30: int32 throughout.
 * NOT BUILT: an in-sweep stop; a Z-drop form of the int32 route of unbanded extension alignments; X-drop.
 * valign_hip_describe: "extend_zdrop_rows" is the key.  On this route "ran_extend" / "ran_extend_align" are "rows" with the
 * geometry beside them, "ran_extend_zdrop" is Z and "extend_zdrop_skipped_waves" is 0 -- the route has no strips.
 * tests/extend_zdrop_ref.py (band_width = 0) restates the records, tests/extend_align_ref.py on the reads cut at T the alignments. */
int valign_hip_set_extend_zdrop_rows(valign_hip_engine *e, int on);

/* Page-lock a host range and map it for the device (hipHostRegister behind a C symbol, so that an FFI caller needs no
 * HIP binding).  valign_hip_align_host into result buffers that lie inside a registered range -- or inside memory the
 * caller page-locked itself -- skips the library's pinned staging and its host-side copy: the device's copy engine
 * writes the caller's buffers directly (the flat layout IS the device layout).  Register once, reuse the buffers;
 * registering costs about a second per GB.  Unregister (with the pointer given to register) before freeing the memory.   */
int valign_hip_host_register(void *ptr, unsigned long long bytes);
int valign_hip_host_unregister(void *ptr);

/* Host-pointer score path (valign_hip_score_host / score_alignments): 1 (default) = the sequences cross PCIe as 4-bit
 * base classes, two per byte, and are expanded to one canonical byte per class in device memory -- the kernels only
 * ever look at the class of a base (DefaultKernel.h:43-60), so scores are identical; 0 = raw ASCII.  Plugin key:
 * host_packing.  Alignments always travel as the caller's bytes (they are copied into the result rows).                 */
int valign_hip_set_host_packing(valign_hip_engine *e, int mode);

/* score_alignments: 1 (default) = the recurrences run on packed half floats wherever every cell provably stays a small
 * integer (exact, bit-identical scores; v_pk_maximum3_f16 saves instructions), 0 = integer cells only.  Plugin key:
 * half_float_cells.                                                                                                      */
int valign_hip_set_half_float_cells(valign_hip_engine *e, int mode);

/* JSON description of what a call with this opt would launch (geometry, LDS, grid).  "score_cells" is a prediction for a
 * device-resident call of n pairs; "ran_score_cells" (f16 / int16 / int32, joined with '+' where a length-sorted call
 * mixed them) and "ran_align_fill" (the alignment path and fill kernel: fused_tag, tag_prof_key, ..., strip, strip_wide,
 * strip_ckpt) report what the engine's last score / alignment call actually launched ("none" before any);
 * "ran_score_geometry" / "ran_align_geometry" name the compiled geometry, "GxK" (group lanes x rows per lane), whose kernel
 * the last register-sweep score launch / the last register-path fill launch ran -- the engine's own, its latency plan's or the
 * full geometry a fallback kernel moved the call to -- and are "none" before any and for every other route;
 * "ran_placed_geometry" / "ran_subopt_geometry" / "ran_extend_geometry" name, in the same way, the geometry whose kernel the last
 * placed-score / suboptimal-score / extension-score register sweep ran -- the engine's own or, where that one carries no kernel
 * for the track and gap form, the full geometry the call was moved to (the key / rows rule is asked again for its rows per lane)
 * -- and are "none" before any such call, after a refused one, and for the strip, chain and wide routes; the forward sweep of a
 * spanned call sets "ran_placed_geometry" like any placed call (the reverse sweep's child engine is not reported);
 * "ran_score_sym_affine" is present only where the last score call launched the int16 symmetric affine Smith-Waterman kernel,
 * and names the form of its sweep that ran: "max3" (biased cells, three-operand maxima) or "sources" (gap sources);
 * "ran_score_sym_affine_frame", present beside it, names the frame of that sweep: "tilted" (the biased form with free gap
 * extensions) or "plain" (also for the gap-source form); "ran_score_sym_affine_scores", present with them, names where the
 * sweep took its substitution scores from: "row_tables" (the tilted frame with one byte per score, kept in registers) or
 * "lds_profile" (everything else);
 * "align_ptr_bytes_per_pair" / "align_ckpt_bytes_per_pair" are the pointer-stream and checkpoint bytes a pair holds in the plan
 * of the last alignment call, "align_scratch_bytes" the pointer scratch the engine holds after it.
 * "ran_result_format" is "rows" or "cigar" for the last alignment call, "cigar_d2h_bytes" what the last
 * valign_hip_align_cigar_host call copied back, "cigar_rows_scratch_bytes" the rows scratch of the compact format.
 * "ran_cigar_lanes" is the lane group per pair the CIGAR encoder of the last valign_hip_align_cigar_*, _align_span_* or
 * _align_extend_* call ran on: 16 (min(R, F) <= 256) or 64 -- for a spanned call those of the window that was walked, R x
 * span_ref_length --, 0 before any such call and after one that was refused or launched nothing.
 * "ran_placed" is what the last placed-score call ran: key / rows / strip / chain / wide ("none" before any, or when it was
 * refused); "band_placed" is the key of valign_hip_set_band_placed, "placed_wide" that of valign_hip_set_placed_wide, "extend_wide" that of valign_hip_set_extend_wide.  "ran_span", "span_ref_length" and "span_scratch_bytes"
 * belong to the spanned scores, "ran_subopt", "subopt_scratch_bytes" and "subopt_ring_cols" to the suboptimal scores,
 * "ran_extend_align", "ran_extend_align_geometry" and "extend_align_scratch_bytes" to the extension alignments, above.
 * "extend_band" is the key of valign_hip_set_extend_band and "extend_band_block_rows" the rows of a block of its band;
 * "ran_extend" is "band" after a banded extension call, with "ran_extend_geometry": "none".                                    */
int valign_hip_describe(valign_hip_engine *e, int opt, long long n, char *buf, int cap);

const char *valign_hip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* VALIGN_HIP_H */
