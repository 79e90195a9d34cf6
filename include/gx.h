/*
 * gx.h -- C ABI of genomics-rs_amd: an MI355X (gfx950) drop-in for the
 * affine-gap alignment path of nlaha/genomics-rs.
 *
 * Every entry point replaces one item of the reference's public Rust API
 * (src/lib.rs:3-6 re-exports alignment, config, sequence).  A Rust shim binds
 * these 1:1 with `extern "C"`.  Plain pointers and sizes
 * only; host memory unless a name says `_device`.  All calls return 0 on
 * success or a GX_E* code; gx_last_error() (thread-local) describes the last
 * failure.  The library never aborts the process.
 */
#ifndef GX_H
#define GX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------- */
#define GX_OK 0
#define GX_EINVAL 1       /* bad argument (NULL, size mismatch)                        */
#define GX_ESEQ 2         /* fewer than 2 sequences: the reference panics (algo.rs:169) */
#define GX_ERANGE 3       /* scores/lengths outside the exact int32 device range        */
#define GX_ENOMEM 4       /* device or host allocation failed                           */
#define GX_EHIP 5         /* HIP runtime error                                          */
#define GX_EPANIC 6       /* the reference would panic (retrace, algo.rs:407-408)       */
#define GX_ECAP 7         /* caller buffer too small (needed size reported)             */
#define GX_EIO 8          /* file could not be read                                     */
#define GX_EPARSE 9       /* config could not be parsed                                 */

/* ---- config.rs:6-13  Scores ------------------------------------------ */
typedef struct gx_scores {
    int64_t s_match;
    int64_t s_mismatch;
    int64_t g; /* per-residue gap */
    int64_t h; /* gap opening     */
} gx_scores;

/* ---- algo.rs:25-35  #[repr(C)] AlignmentCell (48 B, same field order) - */
typedef struct gx_cell {
    int64_t insert_score;
    int64_t delete_score;
    int64_t sub_score;
    uint64_t insert_matches;
    uint64_t delete_matches;
    uint64_t sub_matches;
} gx_cell;

/* ---- algo.rs:124-133  #[repr(u8)] AlignmentChoice ---------------------- */
enum {
    GX_MATCH = 0,
    GX_MISMATCH = 1,
    GX_INSERT = 2,
    GX_DELETE = 3,
    GX_OPEN_INSERT = 4,
    GX_OPEN_DELETE = 5
};

/* one element of AlignedSequences.alignment: (AlignmentChoice, usize, usize) */
typedef struct gx_step {
    uint8_t choice;
    uint8_t pad[7];
    uint64_t i;
    uint64_t j;
} gx_step;

/* ---- algo.rs:135-146  AlignedSequences stats (+ where the walk started) - */
typedef struct gx_result {
    int64_t score;
    uint64_t matches;
    uint64_t mismatches;
    uint64_t gap_extensions;
    uint64_t opening_gaps;
    uint64_t n_steps;        /* alignment.len()                                  */
    uint64_t start_i;        /* retrace start cell (algo.rs:306-323)             */
    uint64_t start_j;
    uint64_t max_cell_i;     /* alignment_table's running max cell (algo.rs:258) */
    uint64_t max_cell_j;
    uint64_t matches_at_max; /* alignment_table's second return (algo.rs:279)    */
    int64_t fill_us;         /* device fill time (µs), for the info! log lines    */
    int64_t retrace_us;      /* traceback time (µs)                              */
} gx_result;

typedef struct gx_context gx_context; /* one per GPU (device memory cache + stream) */
typedef struct gx_table gx_table;     /* a device-resident Array2<AlignmentCell>     */

const char* gx_last_error(void);
const char* gx_version(void);

/* Create a context on HIP device `device`. */
int gx_context_create(int device, gx_context** out);
void gx_context_destroy(gx_context* ctx);
/* Release cached device buffers (they are otherwise reused across calls). */
int gx_context_trim(gx_context* ctx);

/* ---- alignment_table (algo.rs:151-156) --------------------------------
 * Fills the table of the first two sequences on the GPU.  The table stays in
 * HBM (the reference's (n+1)x(m+1) 48 B cells need 42.9 GB at 30k).  The
 * three score planes take 12 B/cell as int32, or 3 B/cell as exact per-cell
 * byte differences (untracked tables on the anti-diagonal layout whose scores
 * pass the range proof, gx_plane_bytes_per_cell; untracked global tables also
 * keep values shifted by (i + j) g on the device).  Every export decodes them
 * to the reference's int64 values.  `reverse_sequences` has the semantics of
 * is_match(.., true) (sequence.rs:102-115).  On success *table_out owns the
 * table and *matches_at_max holds the second tuple element.  Passing
 * matches_at_max = NULL skips the running-max/LCS tracking (gx_table_info
 * then reports max cell (0, 0)) unless GX_TABLE_MATCHES is set.
 * flags: GX_TABLE_PLANES keeps the three score planes (needed for export);
 *        GX_TABLE_MATCHES additionally keeps the LCS plane so that the
 *        *_matches fields can be exported (full AlignmentCell fidelity).   */
#define GX_TABLE_PLANES 1u
#define GX_TABLE_MATCHES 2u
int gx_alignment_table(gx_context* ctx, const uint8_t* s1, size_t n, const uint8_t* s2, size_t m,
                       const gx_scores* scores, int is_local, int reverse_sequences, uint32_t flags,
                       gx_table** table_out, uint64_t* matches_at_max);

/* Shape and running-max bookkeeping of a table. */
int gx_table_info(const gx_table* t, uint64_t* n_rows /* n+1 */, uint64_t* n_cols /* m+1 */,
                  uint64_t* max_cell_i, uint64_t* max_cell_j, int64_t* fill_us);

/* Copy the whole table into caller memory as the reference's Array2
 * (column-major `.f()`, element (i,j) at i + j*(n+1), algo.rs:172).
 * Requires GX_TABLE_PLANES (and GX_TABLE_MATCHES for the *_matches fields,
 * which are otherwise written as 0). */
int gx_table_export(const gx_table* t, gx_cell* out, size_t out_cells);

/* Copy one score plane (0 = insert, 1 = delete, 2 = sub) as int64, row-major
 * (i*(m+1)+j) when colmajor = 0, column-major otherwise. */
int gx_table_export_plane(const gx_table* t, int which, int64_t* out, size_t out_cells, int colmajor);

/* Rows row0 .. row0+rows-1 of one score plane as int64, row-major rows x (m+1)
 * (a slice of the table: a 30k x 30k plane is 7.2 GB as int64).  Row 0 and
 * column 0 are the reference's boundary cells (algo.rs:195-220).  which = 3:
 * max_matches of each cell (AlignmentCell::max_matches, algo.rs:113-121; 0 on
 * the boundary), for tables built with GX_TABLE_MATCHES.  No reference
 * counterpart (the reference materialises the whole Array2). */
int gx_table_export_rows(const gx_table* t, int which, size_t row0, size_t rows, int64_t* out, size_t out_cells);

/* Checksums of the three score planes, computed on the device from the
 * stored planes: sums[k] = sum over interior cells (i, j >= 1) of plane k's
 * value * (1 + i*0x9E3779B1 + j*0x85EBCA77) mod 2^64 (k = 0 insert, 1 delete,
 * 2 sub; oracle/gx_oracle.c oracle_align_lean folds the same sums).  Requires
 * GX_TABLE_PLANES.  Verification at sizes where exporting is impractical. */
int gx_table_plane_sums(const gx_table* t, uint64_t sums[3]);

/* ---- retrace (algo.rs:287-291) -----------------------------------------
 * Walks the table and consumes it (the reference moves the Array2 in); the
 * handle is invalid afterwards whatever the return code.  steps[] receives
 * AlignedSequences.alignment in the reference's order (end -> start);
 * cap = n + m + 1 always suffices.  GX_ECAP reports out->n_steps needed.  */
int gx_retrace(gx_table* t, int is_local, gx_step* steps, size_t cap, gx_result* out);

/* Frees a table without retracing. */
void gx_table_free(gx_table* t);

/* ---- fused alignment_table + retrace (main.rs:143-150) ----------------
 * main.rs discards alignment_table's matches_at_max, so the fused paths do
 * not track the running max cell unless asked: with GX_ALIGN_MAX_CELL in
 * `flags` the result's max_cell_i/j and matches_at_max are filled as
 * gx_alignment_table would; otherwise they are 0.                         */
#define GX_ALIGN_MAX_CELL 4u
int gx_align(gx_context* ctx, const uint8_t* s1, size_t n, const uint8_t* s2, size_t m,
             const gx_scores* scores, int is_local, int reverse_sequences, uint32_t flags, gx_step* steps,
             size_t cap, gx_result* out);

/* ---- many independent pairs in one device launch -----------------------
 * Pair p aligns s1[p] (n[p]) with s2[p] (m[p]).  Score planes are not kept
 * (only the traceback codes), so the batch fits HBM.  steps may be NULL
 * (stats only); otherwise steps[p] has caps[p] entries.  flags as gx_align. */
int gx_align_batch(gx_context* ctx, const uint8_t* const* s1, const size_t* n, const uint8_t* const* s2,
                   const size_t* m, size_t npairs, const gx_scores* scores, int is_local, uint32_t flags,
                   gx_step* const* steps, const size_t* caps, gx_result* out);

/* The same over several GPUs: ctxs[0..nctx-1] are contexts created with
 * gx_context_create (one per device; two contexts on one device are allowed).
 * The pairs are shared out by longest-processing-time on n[p] * m[p] cells and
 * each share runs as one gx_align_batch on its own host thread; results land
 * at their pair's index.  SURVEY.md 8(b)'s gx_align_batch(..., ndev) shape; the
 * reference's multi-worker driver is the rayon pool of main.rs:245-261. */
int gx_align_batch_multi(gx_context* const* ctxs, int nctx, const uint8_t* const* s1, const size_t* n,
                         const uint8_t* const* s2, const size_t* m, size_t npairs, const gx_scores* scores,
                         int is_local, uint32_t flags, gx_step* const* steps, const size_t* caps, gx_result* out);

/* ---- device-resident benchmarking path ---------------------------------
 * Stage one pair per slot in HBM once (gx_stage_pairs), then run the hot
 * path (fill with score planes + traceback) on the staged inputs with no
 * host->device traffic.  Used by bench.py; results and flags as gx_align.
 * Batches larger than the free HBM run in chunks (gx_batch_chunks). */
int gx_stage_pairs(gx_context* ctx, const uint8_t* const* s1, const size_t* n, const uint8_t* const* s2,
                   const size_t* m, size_t npairs);
int gx_run_staged(gx_context* ctx, const gx_scores* scores, int is_local, int keep_planes, uint32_t flags,
                  gx_result* out, double* fill_ms_out);
/* nsteps back-to-back passes over the staged pairs, pipelined one pass deep
 * (pass k's traceback labelling on the host overlaps pass k+1's fill on the
 * device).  out = the last pass's results; *fill_ms_out = mean fill time. */
int gx_run_staged_steps(gx_context* ctx, const gx_scores* scores, int is_local, int keep_planes, uint32_t flags,
                        int nsteps, gx_result* out, double* fill_ms_out);
/* flags bit for gx_run_staged(_steps) with keep_planes: after every pass's
 * fill, the plane checksums of gx_table_plane_sums are computed for every
 * staged pair (before the planes are reused); gx_staged_plane_sums returns
 * them as [pass][pair][3] (nsteps * npairs * 3 values).  Verification only. */
#define GX_STAGED_PLANE_SUMS 8u
int gx_staged_plane_sums(const gx_context* ctx, uint64_t* out, size_t cap, size_t* n_values);
/* flags bit for gx_run_staged_steps: the staged pairs are two sets of equal
 * size -- pairs 0 .. P/2-1 and P/2 .. P-1, pair p and p + P/2 of the same
 * shape -- and pass k runs set k % 2 through the same pipeline, so that every
 * pass's device buffers once held the other set's data (a pass that read a
 * previous pass's planes or records would see different values).  Pass k's
 * results, plane sums and (for the last pass of each set) walks land at its
 * set's pair indices; the other set's row of pass k is zero.  The sets must
 * fit one chunk (else GX_EINVAL).  Verification only. */
#define GX_STAGED_ALTERNATE 16u
/* flags bit for gx_run_staged_steps with keep_planes: the last pass's score
 * planes stay on the device, in the format the batch launch stored them
 * (twin plane codes 2 B/cell, compact bytes 3 B/cell or int32; DESIGN.md
 * 4.2, 4.4), until the next staged run and the last gx_staged_table of them
 * is freed.  One chunk only (else GX_EINVAL); such a run does not take the
 * overlapped two-group pipeline, whose buffers alternate. */
#define GX_STAGED_KEEP_PLANES 32u
/* A table of staged pair `pair` from the last GX_STAGED_KEEP_PLANES run: the
 * reference hands alignment_table's Array2 to its caller (algo.rs:172, 281),
 * and this hands over a batch's planes the same way -- gx_table_info,
 * gx_table_export, gx_table_export_plane, gx_table_export_rows and
 * gx_table_plane_sums decode them to the reference's values.  Its alignment
 * is the run's (gx_staged_steps): gx_retrace returns GX_EINVAL.  Free with
 * gx_table_free. */
int gx_staged_table(gx_context* ctx, size_t pair, gx_table** table_out);
/* The alignment (AlignedSequences.alignment) of staged pair `pair` from the
 * last pass of the last gx_run_staged(_steps) call; *n_steps = its length
 * (steps may be NULL to query it). */
int gx_staged_steps(const gx_context* ctx, size_t pair, gx_step* steps, size_t cap, size_t* n_steps);
/* Every pass's results of the last gx_run_staged(_steps) call, [pass][pair]
 * (nsteps * npairs records; `out` of that call is the last pass's row), so
 * that each timed pass can be checked, not only the last.  Verification only. */
int gx_staged_pass_results(const gx_context* ctx, gx_result* out, size_t cap, size_t* n_values);
/* The last fill launch on ctx: its layout (0: anti-diagonal 128-row strips,
 * 1: column step over 64-row strips, 2: the same as core + side waves,
 * 3: anti-diagonal 64-row strips with one row per lane, the latency fill of
 * untracked single pairs), band width (strips per workgroup) and
 * score-plane bytes written per cell (0: none, 12: int32 planes, 3: compact
 * planes -- per-cell byte differences, decoded exactly by the exports, 2:
 * the twin fill's plane codes -- 12 bits a cell since round 6, DESIGN.md
 * 4.4, batches only; reported rounded up: gx_fill_plane_bits gives the exact
 * figure).  No reference counterpart (measurement only). */
int gx_fill_info(const gx_context* ctx, int* layout, int* band_waves, int* plane_bytes_per_cell);
/* Score-plane bits written per cell by the last fill launch (0, 12: twin
 * plane codes, 24: compact bytes, 96: int32 planes, 192: int64 planes), or
 * -1 without a context.  No reference counterpart (measurement only). */
int gx_fill_plane_bits(const gx_context* ctx);
/* The last device walk collected on ctx, out16 = {1 when it was the
 * sequential strip walk of a twin fill without landing columns (else 0 and
 * zeros up to [7]), the walker wave's priority 0..3, 1 when it ran the
 * kernel with the table-driven block chase, blocks the chase took over all
 * pairs, blocks the fixed-point walk took (every pair's first block, and
 * every block the chase gave back), pairs, pair 0's cycles per block in all,
 * and walking; [8..15]: the priorities of the last eight sequential walks
 * launched on ctx, the latest last (-1: none)}.  The policy: priority 0 for
 * a walk with a fill queued behind it on the rotated pipeline and 3
 * elsewhere, the chase for an unpipelined walk of at most 256 pairs;
 * GX_TB_PRIO=0..3 and GX_TB_FAST=0|1 override.  Measurement only. */
int gx_walk_info(const gx_context* ctx, int* out16);
/* The records of that walk as 32-bit words, for comparing two walkers word
 * for word: {pairs, rows per strip}, then per pair {end i, end j, first
 * strip, blocks chased, blocks walked by the fixed point, its 16-bit half of
 * the twin's code plane, strips} and per strip {entry i, entry j, records,
 * active} followed by that strip's records.  Kept only for walks collected
 * under GX_WALK_RECORDS=1 (GX_EINVAL otherwise).  Writes at most cap words
 * and sets *n_words to the count needed.  Verification only. */
int gx_walk_records(const gx_context* ctx, uint32_t* out, size_t cap, size_t* n_words);
/* Chunks of the last gx_run_staged(_steps) / gx_align_batch call: a batch
 * whose device footprint (planes, codes, skeleton) exceeds the free HBM runs
 * as contiguous chunks of pairs through the same device buffers
 * (GX_CHUNK_BYTES overrides the per-chunk byte budget).  Measurement only. */
int gx_batch_chunks(const gx_context* ctx);
/* 1 when the last fill launch on ctx was the twin fill (two pairs per band,
 * one per 16-bit half, packed arithmetic), else 0.
 * Measurement only (GX_TWIN=0 disables it, GX_TWIN=1 forces it where the
 * range bound admits it; by default deep band queues take it). */
int gx_fill_twin(const gx_context* ctx);
/* Rows per lane of the last fill launch when it was the twin fill: 2 (128-row
 * strips) or 4 (256-row strips; GX_TWIN_ROWS=2|4 forces either where it can
 * be launched), 0 for every other fill, -1 without a context.  Measurement only. */
int gx_fill_rows(const gx_context* ctx);
/* 1 when the last fill launch on ctx took its match / mismatch scores from the
 * small-alphabet score tables (at most 4 distinct symbols and scores that fit
 * the tables' bytes; GX_NO_SCORE_TABLE turns them off), 0 when it used the
 * plain match test, -1 without a context.  Measurement only. */
int gx_fill_score_table(const gx_context* ctx);

/* Fill launches per pass of the last staged / batch call: 2 when the pairs
 * ran as two groups whose walks overlap the next pass's fills (a batch of
 * long pairs on the twin fill), else 1. */
int gx_fill_groups(const gx_context* ctx);
/* Which overlapped pipeline the last staged / batch call ran: 2 the rotation
 * of three plane buffers (global batches split in halves; GX_OVERLAP_ROTATE=0
 * turns it off), 1 two group-A buffers and one group-B buffer (local batches,
 * GX_OVERLAP_A splits), 0 none (gx_fill_groups 1), -1 without a context. */
int gx_overlap_scheme(const gx_context* ctx);
/* The rotation's index arithmetic for fill number `fill` = 2 pass + group
 * (host only, no device call).  out7: the FillJob it fills (fill % 3), its
 * fill slot, its walk slot, its stream (0 / 1), the walk whose end its stream
 * waits for on the device (-1: none), the last fill the host has collected
 * and the last walk it has labelled before it enqueues this fill (-1: none). */
int gx_overlap_rotate_plan(int fill, int* out7);
/* Score-plane bytes per cell a batch launch (layout 0, no max tracking)
 * writes with these scores: 3 when the compact format's range proof holds
 * (global mode, g, h <= 0, differences within a signed byte), else 12; -1 on
 * invalid scores.  An upper bound: a launch that takes the twin fill with
 * its plane codes writes 2 (gx_fill_info reports the
 * launch's own figure). */
int gx_plane_bytes_per_cell(const gx_scores* scores, int is_local);

/* The twin fill's int16 admission rule for global batches:
 * *bound receives the largest |value - base| a band of `band_waves` strips can
 * reach with these scores when a twin's two pairs differ by up to col_gap
 * columns; returns 1 when the global twin fill admits the band (bound <
 * 30,000 < 2^15), 0 when it does not, -1 on invalid scores.  Diagnostic
 * (tests/test_twin_bound.py checks the rule against brute-force spreads).
 * No reference counterpart. */
int gx_twin_admission(const gx_scores* scores, int band_waves, int64_t col_gap, int64_t* bound);
/* The same rule for either mode: local batches (is_local = 1) keep plain
 * values relative to the same per-block bases, with the neighbour difference
 * max(|h + g|, U) of the unshifted values and the floor's constants
 * (DESIGN.md 6.7).  Same returns as gx_twin_admission. */
int gx_twin_admission_mode(const gx_scores* scores, int is_local, int band_waves, int64_t col_gap, int64_t* bound);
/* The same rule for a fill with rows_per_lane rows a lane: 2 (128-row strips,
 * the value gx_twin_admission_mode gives) or 4 (the global batch fill's 256-row
 * strips: a strip then spans 320 instead of 192 neighbour steps, DESIGN.md
 * 6.5).  Local fills keep two rows a lane: 0 at four.  -1 on invalid scores or
 * any other rows_per_lane. */
int gx_twin_admission_rows(const gx_scores* scores, int is_local, int band_waves, int64_t col_gap,
                           int rows_per_lane, int64_t* bound);
/* Rows per lane a global staged launch of these pair shapes with planes would
 * take (host rule only, no device; the rule run_fill itself applies, twin
 * pairing and int16 admission included): 4 (256-row strips) or 2; 2 also when
 * the launch would not be the twin fill.  *band_waves (may be NULL) receives
 * the twin fill's band width, 0 when the launch is not the twin fill.
 * grid_cap = the device's CU count (0: 256).  GX_TWIN, GX_TWIN_ROWS,
 * GX_BAND_WAVES, GX_FILL_GRID and GX_LAYOUT act as they do on a launch.  -1 on
 * invalid scores or shapes (every n and m must be >= 1). */
int gx_plan_twin_rows(const gx_scores* scores, const int64_t* n, const int64_t* m, size_t npairs, int grid_cap,
                      int* band_waves);
/* The fill layout a launch of these pair shapes would take (host rule only,
 * no device): 0 = anti-diagonal 128-row strips (batches), 1 = the column
 * step, 3 = skewed 64-row strips (the latency layouts);
 * `track` = an alignment_table call that keeps max_cell / matches_at_max
 * (algo.rs:258-262, 279).  grid_cap = the device's CU count (0: 256).  -1 on
 * invalid arguments.  Diagnostic; no reference counterpart. */
int gx_plan_layout(const gx_scores* scores, int is_local, const int64_t* n, const int64_t* m, size_t npairs,
                   int track, int grid_cap);

/* ---- sequence.rs / config.rs mirrors ----------------------------------- */
/* from_fasta (sequence.rs:45-95) on a file: records are appended to the
 * caller's buffers.  Returns GX_OK and sets *n_records; names/sequences are
 * concatenated into `buf` (cap bytes) with offsets/lengths in the arrays
 * (rec_cap entries).  An unreadable file logs and yields 0 records (the
 * reference swallows the error, sequence.rs:84-86). */
int gx_fasta_load(const char* path, uint8_t* buf, size_t cap, uint64_t* name_off, uint64_t* name_len,
                  uint64_t* seq_off, uint64_t* seq_len, size_t rec_cap, size_t* n_records, size_t* bytes_needed);
/* get_config (config.rs:21-40): reads [scores] s_match, s_mismatch, g, h. */
int gx_config_load(const char* path, gx_scores* out);

/* Display for AlignedSequences (display.rs:9-127) into `out` (NUL-terminated).
 * *needed receives the full length + 1. */
int gx_format_alignment(const uint8_t* s1, size_t n, const uint8_t* s2, size_t m, const gx_step* steps,
                        size_t n_steps, const gx_result* res, char* out, size_t cap, size_t* needed);

/* print_alignment_table + print_scores_table (display.rs:131-220), which the
 * reference's retrace prints to stdout with the table it consumed
 * (algo.rs:438).  Planes are int64 row-major (n+1)x(m+1), as
 * gx_table_export_plane(.., colmajor = 0) writes them (export them before
 * gx_retrace consumes the table).  Empty output when n >= 200 or m >= 2000
 * (the reference only warns then).  color != 0: ANSI styles of the `colored`
 * crate (the reference colours only when stdout is a terminal).  GX_EPANIC
 * where the reference's chars().nth().unwrap() panics (non-ASCII input). */
int gx_format_table(const uint8_t* s1, size_t n, const uint8_t* s2, size_t m, const gx_step* steps, size_t n_steps,
                    const int64_t* insert_plane, const int64_t* delete_plane, const int64_t* sub_plane, int color,
                    char* out, size_t cap, size_t* needed);

/* ---- compare mode (main.rs:216-379) --------------------------------------
 * The reference builds a generalized suffix tree per get_matches call; the
 * quantity it reads off the tree is the longest run of equal bytes along a
 * diagonal of the comparison grid, which the GPU computes directly
 * (DESIGN.md 16).  Input bytes must be above '$' (0x24): at or below it they
 * collide with the reference's terminators ('$', '!') -> GX_EINVAL.
 * Sequences of 2^30 bytes or more -> GX_ERANGE. */

/* One element of the similarity matrix: the tuple (score, len_i, len_j,
 * first_lcs_length) of main.rs:310-315. */
typedef struct gx_compare_cell { uint64_t score, len_i, len_j, first_lcs; } gx_compare_cell;

/* get_lcs(0, 1) (tree.rs:218-281) on a tree holding a then b, on the host with
 * no device: *len = the longest common substring's length L, W = the
 * lexicographically smallest common substring of that length (the DFS visits
 * children in alphabet order, tree.rs:444-464, and keeps the first deepest
 * node), *i / *j = the start of the smallest suffix of a + '$' / b + '!' that
 * begins with W (the first leaf below the node).  L = 0 gives (0, 0, 0). */
int gx_common_substring_host(const uint8_t* a, size_t n, const uint8_t* b, size_t m,
                             uint64_t* i, uint64_t* j, uint64_t* len);
/* The same on the GPU (one sub-problem, no recursion). */
int gx_common_substring(gx_context* ctx, const uint8_t* a, size_t n, const uint8_t* b, size_t m,
                        uint64_t* i, uint64_t* j, uint64_t* len);
/* One matrix element (main.rs:281-315): first_lcs = L of (a, b); score = the
 * sum of L over the traversal that recurses on (a[..i], b[..j]) and
 * (a[i+L..], b[j+L..]) while L > 0.  *n_calls (may be NULL) = get_matches
 * calls (main.rs:267-279), empty pieces included.  ctx = NULL runs the whole
 * recursion on the host solver. */
int gx_compare_pair(gx_context* ctx, const uint8_t* a, size_t n, const uint8_t* b, size_t m,
                    gx_compare_cell* out, uint64_t* n_calls);
/* The similarity matrix (main.rs:241-316): out[j * nseq + i] for i <= j, the
 * other half zero as the reference leaves it.  The sequences are staged on
 * the device once and the recursions of all pairs advance level by level,
 * one batch of launches per level.  ctx = NULL: host solver only. */
int gx_compare_matrix(gx_context* ctx, const uint8_t* const* seqs, const size_t* lens, size_t nseq,
                      gx_compare_cell* out);
/* The last compare call on ctx: sub-problems answered by the kernels, by the
 * host solver (those below GX_COMPARE_HOST_CELLS cells with everything under
 * them, and the overflowed ones), sub-problems whose candidate buffer
 * overflowed (GX_COMPARE_CAND_CAP), and levels that launched.  No reference
 * counterpart (measurement only). */
int gx_compare_info(const gx_context* ctx, uint64_t* gpu_subproblems, uint64_t* host_subproblems,
                    uint64_t* overflowed, uint64_t* levels);
/* Batches of launches (run, combine, candidate) of the last compare call on
 * ctx: one per level, more where a level's sub-problems exceed the budget of
 * tile elements or of candidate slots of one batch.  Measurement and tests
 * only. */
int gx_compare_batches(const gx_context* ctx, uint64_t* batches);
/* Rows per segment of the run kernel's tiles: diagonals are
 * cut every this many rows of a.  Measurement and tests only. */
int gx_compare_segment_height(void);
/* Byte compares and device time (ms) of the run-kernel launches of the last
 * compare call on ctx.  Measurement only. */
int gx_compare_run_stats(const gx_context* ctx, uint64_t* byte_compares, double* run_ms);
/* L and the number of (i, j) starts of common substrings of that length, from
 * the host solver: what the candidate buffer of a sub-problem would have to
 * hold (the measurement behind GX_COMPARE_CAND_CAP's default). */
int gx_common_substring_candidates_host(const uint8_t* a, size_t n, const uint8_t* b, size_t m,
                                        uint64_t* len, uint64_t* n_candidates);

/* ---- suffix-tree mode (main.rs:154-215) ----------------------------------
 * What compute_stats (tree.rs:740-803) reads off the suffix tree of
 * t = s + '$' is a function of the suffix array SA and the LCP array of t
 * (suffixes in plain byte order, LCP[0] = 0), which the GPU builds with radix
 * sorts and scans instead of a tree.  Input bytes must be above
 * '$' (0x24) -> GX_EINVAL otherwise; n >= 2^30 -> GX_ERANGE.  N = n + 1. */

/* TreeStats (tree.rs:30-39) without the BWT; average_string_depth =
 * string_depth_sum / num_internal as f64 (NaN for 0 / 0).  num_internal counts
 * the non-root internal nodes, num_nodes = num_internal + num_leaves + 1,
 * longest_repeat_start is the reference's 1-based leaf id (0: no repeat). */
typedef struct gx_suffix_stats {
    uint64_t num_internal, num_leaves, num_nodes, string_depth_sum,
             max_string_depth, longest_repeat_start, longest_repeat_len;
} gx_suffix_stats;
/* compute_stats(0) on a tree holding s.  bwt (n+1 bytes), sa, lcp (n+1 uint32
 * each) may be NULL.  ctx = NULL: host solver, no device.  With a context,
 * inputs shorter than GX_SUFFIX_HOST_BELOW bytes (default 4096, the lower
 * bracket of the measured crossing: DESIGN.md 17.3) and the empty input go to
 * the host solver too.  When the doubling's bound on max LCP puts the LCP
 * kernel's work, (N / C) * max LCP / 8 eight-byte compares, above
 * GX_SUFFIX_LCP_BUDGET (default 2^40: unary or long-period input of tens of Mi
 * bases), the LCP array and the statistics are finished on the host from the
 * device's suffix array. */
int gx_suffix_tree_stats(gx_context* ctx, const uint8_t* s, size_t n, gx_suffix_stats* out,
                         uint8_t* bwt, uint32_t* sa, uint32_t* lcp);
/* The last suffix-tree call on ctx: sorts (prefix-doubling rounds, the first
 * included), radix passes that ran, and the device time (ms) of the sorts, the
 * LCP kernel and the statistics fold.  All zero when the host solver answered.
 * Measurement only. */
int gx_suffix_info(const gx_context* ctx, uint64_t* doubling_rounds, uint64_t* sort_passes,
                   double* sort_ms, double* lcp_ms, double* fold_ms);
/* The radix passes of the last suffix-tree call on ctx by digit: passes[p] =
 * the passes that sorted on key bits 8p .. 8p+7, over all rounds, round 0
 * included (their sum is sort_passes).  A digit that is the same in every key
 * of a round is skipped there.  Round 0's keys are text bytes and as a rule
 * differ in all eight digits, so it adds one to every entry; from round 1 on
 * the keys are rank pairs, p = 0..3 the low rank and p = 4..7 the high one, so
 * a pass on rank bits 16-23 shows as passes[2], passes[6] >= 2.  All zero
 * when the host solver answered.  Measurement and tests. */
int gx_suffix_digit_passes(const gx_context* ctx, uint64_t passes[8]);
/* Items per workgroup of the sort and scan kernels, text positions per lane of
 * the LCP kernel, LCP entries per block of the fold.  Tests only. */
int gx_suffix_tile(int* sort_items_per_wg, int* lcp_chunk, int* fold_block);
/* Display for TreeStats (display.rs:8-38) byte for byte: leading newline,
 * 12-space indentation, the BWT cut to 100 bytes with "... (truncated)".
 * GX_ECAP reports *needed (with the terminating NUL). */
int gx_format_suffix_stats(const gx_suffix_stats* st, const uint8_t* bwt, size_t bwt_len,
                           char* out, size_t cap, size_t* needed);

/* ---- search mode (no counterpart in the reference's main.rs) ----------------
 * "Where does this string occur?", for a batch of patterns, on the suffix
 * array of t = s + '$' kept on the device.  Conventions as
 * suffix-tree mode: N = n + 1, suffixes in plain unsigned byte order, text and
 * pattern bytes above '$' (0x24).  A pattern P of m bytes, 0 <= m <= 65,535:
 *   lo          the number of suffixes smaller than P (one that has P as a
 *               prefix is not smaller)
 *   count       the number of suffixes that have P as a prefix: SA[lo .. lo +
 *               count), overlapping occurrences included
 *   prefix_len  the longest prefix of P that occurs in t (m when count > 0)
 *   prefix_pos  one position of it: SA[lo] when count > 0; otherwise, with
 *               a = lcp(P, SA[lo - 1]) and b = lcp(P, SA[lo]) (0 when lo = N),
 *               SA[lo - 1] if a >= b, else SA[lo]; 0 when prefix_len = 0
 * m = 0: lo = 0, count = N, prefix_len = 0, prefix_pos = SA[0] = n. */
typedef struct gx_suffix_index gx_suffix_index;   /* text + suffix array, device-resident (host with ctx = NULL) */
typedef struct gx_search_hit { uint32_t lo, count, prefix_len, prefix_pos; } gx_search_hit;

/* The index of s.  With a context it lives in device memory (N + 16 text bytes
 * and 4 N suffix-array bytes from the context's pool, held until
 * gx_suffix_index_free) and every search on it runs on the device; the array
 * of an input shorter than GX_SUFFIX_HOST_BELOW comes from the host solver and
 * is uploaded.  No LCP array is built (GX_SUFFIX_LCP_BUDGET does not apply).
 * ctx = NULL: index and searches on the host, no device.  Errors as
 * gx_suffix_tree_stats.  Indexes are freed before their context is destroyed;
 * several may live on one context. */
int  gx_suffix_index_build(gx_context* ctx, const uint8_t* s, size_t n, gx_suffix_index** out);
void gx_suffix_index_free(gx_suffix_index* idx);
/* n, whether the index is device-resident, and the device bytes it holds. */
int  gx_suffix_index_info(const gx_suffix_index* idx, uint64_t* n, int* on_device, uint64_t* device_bytes);
/* The suffix array, n + 1 entries. */
int  gx_suffix_index_export(const gx_suffix_index* idx, uint32_t* sa /* n+1 */);
/* Pattern p is patterns[offsets[p] .. offsets[p + 1]).  hits[p] as above.  With
 * positions, pattern p reports q_p = min(count_p, max_hits) of its occurrences,
 * SA[lo_p .. lo_p + q_p) sorted ascending, at positions[hit_offsets[p] ..
 * hit_offsets[p + 1]).  GX_EINVAL: a pattern byte at or below '$' (the message
 * names pattern and offset), offsets not non-decreasing from 0.  GX_ERANGE: a
 * pattern longer than 65,535 bytes; total pattern bytes plus npat, or total
 * reported positions, at or above 2^32.  GX_ECAP: positions_cap is below the
 * total (named in gx_last_error()): hits[] and hit_offsets[] are complete,
 * positions[] is untouched. */
int  gx_suffix_index_search(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets /* npat+1 */,
                            size_t npat, gx_search_hit* hits /* npat */, uint32_t max_hits,
                            uint32_t* positions /* may be NULL: counts only */, size_t positions_cap,
                            uint64_t* hit_offsets /* npat+1, may be NULL iff positions is NULL */);
/* The last search on ctx: 8-byte compare steps of the interval kernel, its
 * device time (ms) and that of the locate step (clamp, scan and gather; 0 for
 * counts only).  Measurement and tests. */
int  gx_search_info(const gx_context* ctx, uint64_t* word_compares, double* search_ms, double* locate_ms);

/* ---- approximate search: at most k substitutions -------------
 * Conventions as above; one k for the whole call, 0 <= k <= GX_APPROX_MAX_K,
 * and every pattern has m >= k + 1 bytes.  An occurrence of P is a start i
 * with 0 <= i and i + m <= n (the window never touches '$') and
 * d(i) = |{ j : s[i + j] != P[j] }| <= k.  Substitutions only: no indels.
 *   count       the number of occurrences, overlapping ones included; max_hits
 *               does not reduce it
 *   best_dist   the smallest d(i) over them, 0xFFFFFFFF when count = 0
 *   best_pos    the smallest i with d(i) = best_dist, 0 when count = 0
 *   candidates  the seed hits verified for this pattern (the work measure)
 * P is cut into k + 1 pieces, piece j = [floor(j m / (k + 1)), floor((j + 1) m
 * / (k + 1))); an occurrence leaves at least one piece intact, so it is among
 * the exact hits of the pieces (the seeds), shifted by the piece's start; the
 * first intact piece alone reports it. */
#define GX_APPROX_MAX_K 8
typedef struct gx_approx_hit { uint32_t count, best_dist, best_pos, candidates; } gx_approx_hit;

/* hits[p] as above.  With positions, pattern p reports q_p = min(count_p,
 * max_hits) occurrences at positions[hit_offsets[p] .. hit_offsets[p + 1]),
 * ascending, with their distances beside them in distances[].  When count_p >
 * max_hits they are the first max_hits in candidate order (piece index, then
 * suffix-array order within the piece's interval), then sorted; the host index
 * and the device keep the same ones.  Errors as gx_suffix_index_search, and
 * GX_EINVAL: k > GX_APPROX_MAX_K, a pattern shorter than k + 1 bytes (named),
 * distances NULL with positions.  GX_ERANGE: npat (k + 1) + 1 at or above
 * 2^32; the seed hits of the batch come to more than GX_APPROX_CAND_BUDGET
 * (environment, read on every call; default 2^27, at most 2^31; about 12 pooled
 * device bytes a candidate): nothing is verified and of hits[] only the
 * candidates fields are written; split the batch, lower k or raise the budget.
 * GX_ECAP: hits[] and hit_offsets[] are complete, positions[] and distances[]
 * are untouched. */
int  gx_suffix_index_search_approx(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets /* npat+1 */,
                                   size_t npat, uint32_t k, gx_approx_hit* hits /* npat */, uint32_t max_hits,
                                   uint32_t* positions /* may be NULL: counts only */,
                                   uint8_t* distances /* may be NULL iff positions is NULL */, size_t positions_cap,
                                   uint64_t* hit_offsets /* npat+1, may be NULL iff positions is NULL */);
/* The last approximate search on ctx: the seed hits of the batch, the 8-byte
 * steps of the verify kernel, device time (ms) of pieces, seeds, total and
 * candidate offsets, and of verify and compact.  Measurement and tests. */
int  gx_approx_info(const gx_context* ctx, uint64_t* candidates, uint64_t* word_compares, double* seed_ms,
                    double* verify_ms);

/* ---- edit search: at most k differences ----------------------
 * Conventions as above (one k, 0 <= k <= GX_APPROX_MAX_K, every pattern of
 * k + 1 bytes or more), and m <= GX_EDIT_MAX_M: one lane's work in one launch
 * stays at or below m (2k + 1), about 70,000 cell updates.  ed is the
 * unit-cost Levenshtein distance: a substitution, an insertion and a deletion
 * cost 1 each.  For an end 0 <= e <= n,
 *   E(e) = min over 0 <= b <= e of ed(P, s[b .. e))            (Sellers)
 * An occurrence of P is an end e with E(e) <= k, reported as that exclusive
 * end; its start is b(e) = max{ b : ed(P, s[b .. e)) = E(e) }, the shortest
 * window, with e - b(e) in [m - k, m + k].  A window never contains '$'.
 *   count       the number of ends with E(e) <= k; max_hits does not reduce it
 *   best_dist   the smallest E(e), 0xFFFFFFFF when count = 0
 *   best_end    the smallest e with E(e) = best_dist, 0 when count = 0
 *   candidates  the seed hits verified for this pattern (the work measure)
 * At k = 0 an occurrence is pos + m for each exact position pos, its start pos.
 * The seeds are the k-mismatch search's: k edits leave one of k + 1 pieces
 * intact.  Each seed hit is verified on the 2k + 1 diagonals around its own;
 * E(e) is the minimum over the seed hits that report e. */
#define GX_EDIT_MAX_M 4096
typedef struct gx_edit_hit { uint32_t count, best_dist, best_end, candidates; } gx_edit_hit;

/* hits[p] as above.  With ends, pattern p reports q_p = min(count_p, max_hits)
 * occurrences, its q_p smallest ends, ascending, at [hit_offsets[p],
 * hit_offsets[p + 1]) of ends[], distances[] (E(e)) and, unless it is NULL,
 * starts[] (b(e)).  Errors as gx_suffix_index_search_approx (GX_EINVAL also for
 * starts without ends), and GX_ERANGE: a pattern longer than GX_EDIT_MAX_M
 * (named); the seed hits of the batch, or the ends its seed hits report before
 * equal ends are merged (at most 2k + 1 a seed hit), come to more than
 * GX_APPROX_CAND_BUDGET (about 16 pooled device bytes a seed hit and 29 an
 * unmerged end): nothing further runs and of hits[] only the candidates fields
 * are written.  GX_ECAP: hits[] and hit_offsets[] are complete, ends[],
 * distances[] and starts[] are untouched. */
int  gx_suffix_index_search_edit(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets /* npat+1 */,
                                 size_t npat, uint32_t k, gx_edit_hit* hits /* npat */, uint32_t max_hits,
                                 uint32_t* ends /* may be NULL: counts only */,
                                 uint8_t* distances /* may be NULL iff ends is NULL */,
                                 uint32_t* starts /* may be NULL: no start is computed */, size_t positions_cap,
                                 uint64_t* hit_offsets /* npat+1, may be NULL iff ends is NULL */);
/* The last edit search on ctx: the seed hits of the batch, the ends they
 * reported before equal ends were merged, the cell updates of the verify kernel
 * (at most sum_p candidates_p m_p (2k + 1)), and device time (ms) of the seed
 * stages, of the verify kernel, and of scan, emit, sort, merge, scatter and
 * starts.  Measurement and tests. */
int  gx_edit_info(const gx_context* ctx, uint64_t* candidates, uint64_t* pre_dedupe_ends, uint64_t* cell_updates,
                  double* seed_ms, double* verify_ms, double* dedupe_ms);

/* ---- matching statistics and maximal exact matches ------------
 * Long queries against the index: where a genome or a contig agrees with the
 * text.  Conventions as above (t = s + '$', N = n + 1, unsigned byte order, every
 * query byte above '$').  A call takes a batch of queries concatenated like
 * patterns, of any length: query c is queries[offsets[c] .. offsets[c + 1]), of
 * length m_c, and its positions j are relative to its own start.  The total
 * query bytes stay below 2^32 - 2064: the device's offsets and scans are 32-bit
 * and need room for the 16 bytes of padding and a scan tile (2,048) of rounding.
 *
 * Matching statistics of position j of query c, w = min(max_len, m_c - j):
 *   len     the longest prefix of Q_c[j .. j + w) that occurs in s
 *   lo, count  the suffix-array interval of that prefix: exactly the suffixes
 *           that have Q_c[j .. j + len) as a prefix
 *   pos     SA[lo]
 * and len = 0 gives lo = 0, count = N, pos = SA[0] = n, as m = 0 above.  A lane
 * compares up to w bytes a probe: max_len bounds its work.
 *
 * A MEM of query c is (tpos = i, qpos = j, len) with len >= min_len,
 * s[i .. i + len) = Q_c[j .. j + len), left-maximal (i = 0 or j = 0 or
 * s[i - 1] != Q_c[j - 1]) and right-maximal (i + len = n or j + len = m_c or
 * s[i + len] != Q_c[j + len]).  A match never contains '$' and never crosses
 * into a neighbouring query.  Every such triple is reported exactly once,
 * overlapping ones and those on one diagonal included; within a query they are
 * ordered by qpos, then tpos.  The candidates of a query are the (i, j) pairs
 * examined for it: every occurrence in s of every min_len-mer of the query. */
typedef struct gx_match_stat { uint32_t len, lo, count, pos; } gx_match_stat;
typedef struct gx_mem        { uint32_t qpos, tpos, len; } gx_mem;

/* stats[offsets[c] + j] for position j of query c.  Errors: GX_EINVAL (a query
 * byte at or below '$', query and offset named; bad offsets; max_len = 0; NULL
 * stats), GX_ERANGE (total query bytes + 2064 at or above 2^32, as above). */
int  gx_suffix_index_match_stats(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets /* nq+1 */,
                                 size_t nq, uint32_t max_len, gx_match_stat* stats /* offsets[nq] entries */);
/* The MEMs of query c at [mem_offsets[c], mem_offsets[c + 1]) of mems[];
 * candidates[c] as above.  mems = NULL: counts only (mem_offsets and candidates).
 * Errors as above (min_len = 0, NULL mem_offsets: GX_EINVAL), and GX_ERANGE: the
 * candidates of the batch come to more than GX_APPROX_CAND_BUDGET (read on every
 * call; 12 pooled device bytes a candidate, 36 a kept pair): nothing further runs and only
 * candidates[] is written.  GX_ECAP: mems_cap is below the total (named);
 * mem_offsets[] and candidates[] are complete, mems[] is untouched. */
int  gx_suffix_index_mems(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets /* nq+1 */,
                          size_t nq, uint32_t min_len, gx_mem* mems /* may be NULL: counts only */,
                          size_t mems_cap, uint64_t* mem_offsets /* nq+1 */, uint64_t* candidates /* nq, may be NULL */);
/* The last matching-statistics or MEM call on ctx: candidate pairs, kept
 * (left-maximal) pairs, the 8-byte compare steps of its kernels, and device time
 * (ms) of the matching-statistics kernel, of the seed stages (interval kernel,
 * scan, keep, counts) and of emit, sort and pack.  What did not run is 0.
 * Measurement and tests. */
int  gx_match_info(const gx_context* ctx, uint64_t* candidates, uint64_t* kept, uint64_t* word_compares,
                   double* stats_ms, double* seed_ms, double* emit_ms);

/* ---- banded affine-gap alignment and CIGARs of reported hits --
 * A hit is (p, b, e): pattern P_p of m bytes and the window s[b .. e) of
 * w = e - b bytes, 0 <= b <= e <= n.  For each hit the call runs the
 * reference's global alignment (alignment_table(is_local = false), then retrace,
 * algo.rs:151-441) with s1 = the window (index i) and s2 = the pattern (index
 * j), on the cells with |j - i| <= band alone: every plane of a cell outside the
 * band reads as the reference's negative infinity, the boundary cells (i, 0) and
 * (0, j) inside it are the reference's.  The retrace starts at (w, m), takes in
 * every cell the first of S, I, D at the cell's maximum, and labels and counts
 * its steps as the reference does.  Whenever the reference's own retrace path
 * stays inside the band, record and steps are the reference's.  Insert and
 * OpenInsert consume a pattern byte (the CIGAR's I, the read being the query),
 * Delete and OpenDelete a text byte (D); a diagonal step is an M.
 *
 * hit_offsets, starts and ends are what gx_suffix_index_search_edit returns
 * (npat + 1 offsets; pattern p's hits at [hit_offsets[p], hit_offsets[p + 1])),
 * or the exact or k-mismatch search's positions with ends = position + m, or the
 * caller's own.  out[h] is hit h's record.  Its runs, len << 4 | op with M = 0,
 * I = 1, D = 2, in pattern order, are cigar[cigar_offsets[h] ..
 * cigar_offsets[h + 1]); cigar = NULL asks for the records and the offsets only.
 * A host index (ctx = NULL at its build) runs on the host.
 *
 * Errors, in this order.  GX_EINVAL: idx, offsets, hit_offsets, scores or
 * cigar_offsets is NULL; band above GX_EXTEND_MAX_BAND.  GX_ERANGE: a score above
 * GX_EXTEND_MAX_SCORE in magnitude (int32 is exact below it).
 * Then the batch checker of the searches (a pattern longer than GX_EDIT_MAX_M:
 * GX_ERANGE).  GX_EINVAL: hit_offsets does not start at 0 or decreases;
 * GX_ERANGE: 2^32 hits or more; GX_EINVAL: starts, ends or out is NULL with a
 * hit; a hit with e < b, e > n or |w - m| > band (hit and pattern named).  After
 * the run, GX_ERANGE: 2^32 runs or more; GX_ECAP: cigar_cap is below the total
 * (named): out[] and cigar_offsets[] are complete, cigar[] is untouched. */
#define GX_EXTEND_MAX_BAND 15
#define GX_EXTEND_MAX_SCORE 32767
typedef struct gx_extend_hit {
    int32_t score; uint32_t n_steps;
    uint32_t matches, mismatches, opening_gaps, gap_extensions; /* as retrace counts them */
    uint32_t identities;  /* diagonal steps with s1[i-1] == s2[j-1] */
    uint32_t cigar_len;   /* runs */
} gx_extend_hit;
int  gx_suffix_index_extend(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets /* npat+1 */,
                            size_t npat, const uint64_t* hit_offsets /* npat+1 */, const uint32_t* starts,
                            const uint32_t* ends, const gx_scores* scores, uint32_t band,
                            gx_extend_hit* out /* nhits */, uint32_t* cigar /* may be NULL */, size_t cigar_cap,
                            uint64_t* cigar_offsets /* nhits+1 */);
/* The last extend call on ctx: its hits, the cell updates of the fill (the
 * cells of every hit's table inside the band, at most sum (w + 1)(2 band + 1)),
 * the bytes of trace of its largest launch, its launches (a batch whose trace
 * exceeds GX_EXTEND_TRACE_BYTES, read on every call, runs in chunks), and device
 * time (ms) of the fill and of walk, scan and emit.  Measurement and tests. */
int  gx_extend_info(const gx_context* ctx, uint64_t* hits, uint64_t* cell_updates, uint64_t* trace_bytes,
                    uint64_t* chunks, double* fill_ms, double* walk_ms);

/* ---- colinear chains of a long query's anchors -----------------
 * A batch of nq queries' anchors: query c's are anchors[anchor_offsets[c] ..
 * anchor_offsets[c + 1]), strictly ascending by (qpos, tpos) within a query,
 * which is the order gx_suffix_index_mems writes.  The call reads no text and no
 * index: an anchor need not be a match.  Indices below are anchor numbers within
 * the query, from 0.
 *
 * For anchors a < b of one query, dq = q_b - q_a and dt = t_b - t_a (signed):
 *   a is eligible for b iff b - a <= max_pred, 1 <= dq <= max_gap,
 *     1 <= dt <= max_gap and |dq - dt| <= max_drift
 *   ext(a, b) = f(a) + w_match min(len_b, dq, dt) - w_drift |dq - dt|
 *   f(b) = max(w_match len_b, max over eligible a of ext(a, b))
 *   pred(b) = the eligible a at that maximum, the largest a among equal ext, and
 *     only where the maximum is strictly above w_match len_b; GX_CHAIN_NONE
 *     otherwise, and b is a root.
 * pred makes a forest.  Every tree gives at most one chain: its end e is the
 * tree's anchor of largest f (the smallest index among equals), the chain is the
 * path from the root to e, and it is reported iff f(e) >= min_score.  A query's
 * chains are disjoint and ordered by root.  members[member_off .. member_off +
 * n_anchors) of a chain are its anchor numbers ascending; the members of
 * successive chains follow each other in chain order.  Query c's chains are
 * chains[chain_offsets[c] .. chain_offsets[c + 1]).
 *
 * ctx = NULL runs the host solver, with the same results field by field.
 * scores[] and preds[] (f and pred of every anchor; either may be NULL) are in
 * the order of anchors[].  chains = NULL asks for the counts only.
 *
 * Errors, in this order.  GX_EINVAL: anchor_offsets, chain_offsets or
 * members_total is NULL; a parameter out of range (named).  GX_ERANGE: 2^32 - 2049
 * queries or more.  GX_EINVAL: anchor_offsets does not start at 0 or decreases;
 * members NULL with chains.  GX_ERANGE: more anchors than GX_APPROX_CAND_BUDGET
 * (read on every call; up to 100 pooled device bytes an anchor).  GX_EINVAL:
 * anchors NULL with an anchor.
 * Then per anchor in turn: GX_EINVAL len = 0; GX_ERANGE qpos + len or tpos + len
 * at or above 2^32; GX_EINVAL an anchor not above its predecessor in (qpos, tpos)
 * (query and anchor named); and at a query's end GX_ERANGE w_match sum(len) at or
 * above 2^31 (query named).  Nothing runs in these cases.  After the run GX_ECAP:
 * chains_cap, then members_cap, below the total (named): chain_offsets,
 * members_total, scores and preds are complete, chains and members untouched. */
#define GX_CHAIN_NONE 0xFFFFFFFFu
#define GX_CHAIN_MAX_PRED 256
#define GX_CHAIN_MAX_WEIGHT 1024
#define GX_CHAIN_MAX_GAP (1u << 20)
#define GX_CHAIN_DEFAULT_W_MATCH 8
#define GX_CHAIN_DEFAULT_W_DRIFT 1
#define GX_CHAIN_DEFAULT_MAX_GAP 5000
#define GX_CHAIN_DEFAULT_MAX_DRIFT 500
#define GX_CHAIN_DEFAULT_MAX_PRED 64
#define GX_CHAIN_DEFAULT_MIN_SCORE 0
typedef struct gx_chain_params {
    uint32_t w_match, w_drift, max_gap, max_drift, max_pred;
    int32_t min_score;
} gx_chain_params;
typedef struct gx_chain {
    uint64_t member_off;
    int32_t score;               /* f(end) */
    uint32_t n_anchors, root, end;
    uint32_t qstart, tstart;     /* of the root */
    uint32_t qend, tend;         /* start + len of the end */
} gx_chain;
int  gx_chain_anchors(gx_context* ctx /* NULL: host */, const gx_mem* anchors, const uint64_t* anchor_offsets /* nq+1 */,
                      size_t nq, const gx_chain_params* params /* NULL: the defaults */,
                      int32_t* scores /* may be NULL */, uint32_t* preds /* may be NULL */,
                      gx_chain* chains /* may be NULL: counts only */, size_t chains_cap, uint32_t* members,
                      size_t members_cap, uint64_t* chain_offsets /* nq+1 */, uint64_t* members_total);
/* The last chain call on ctx: its anchors, segments (a query's anchors are cut
 * wherever qpos advances by more than max_gap: nothing chains across), the pairs
 * (a, b) of one segment with 1 <= b - a <= max_pred that the score kernel
 * evaluated, its reported chains, and device time (ms) of flags, scan and score
 * and of best, heads, scans and walk.  What did not run is 0.  Measurement and
 * tests. */
int  gx_chain_info(const gx_context* ctx, uint64_t* anchors, uint64_t* segments, uint64_t* pair_evals, uint64_t* chains,
                   double* score_ms, double* chain_ms);

/* ---------------------------------------------------------------------------
 * Search mode on both strands.
 *
 * strand_comp, the complement table: an involution over all 256 bytes, IUPAC in
 * both cases (A-T, C-G, R-Y, K-M, B-V, D-H; S, W, N and every other byte, U
 * included, map to themselves), so a byte above '$' stays above it.
 * rc(P)[j] = strand_comp(P[m - 1 - j]).
 *
 * The item batch of a caller's batch of n patterns P_0 .. P_{n-1} (T bytes):
 *   GX_STRAND_FWD   the batch itself
 *   GX_STRAND_REV   n items, item p = rc(P_p)
 *   GX_STRAND_BOTH  2n items: item p = P_p, item n + p = rc(P_p), bytes back to
 *                   back in that order (off'[p] = off[p], off'[n + p] = T + off[p])
 *
 * The contract of every _strands call: it returns, in every output array, every
 * count and its return code, what the call without the suffix returns on the
 * item batch of gx_revcomp_batch with the same remaining arguments, on the
 * device and on a host index.  So
 *   - every per-pattern array (hits, hit_offsets, candidates, mem_offsets, stats,
 *     ...) has one entry per item: n for FWD and REV, 2n for BOTH; extend's
 *     hit_offsets has items + 1 entries, and the hits of item n + p are aligned
 *     against rc(P_p), which is what SAM reports for a reverse-strand read;
 *   - positions, ends and starts are coordinates of the forward text;
 *   - a reverse item's MEM qpos and the positions of match_stats are coordinates
 *     of rc(Q): the same bases sit at m - qpos - len in the caller's query;
 *   - a pattern equal to its own reverse complement reports in both items,
 *     nothing is merged;
 *   - GX_APPROX_CAND_BUDGET and the extend trace budget apply to the item batch.
 * On a context the caller's bytes are copied to the device once, as without
 * strands, and a kernel writes the reverse items behind them.
 *
 * Refusals, in this order: GX_EINVAL when strands is not 1, 2 or 3; what the
 * call without the suffix refuses of the caller's batch, codes, texts and order
 * unchanged, pattern numbers the caller's; then everything as the call without
 * the suffix on the item batch: where a text names a pattern it is the item
 * number.  One refusal is new: GX_ERANGE "strands: ..." when the item batch (the
 * doubled bytes and items) fails the 32-bit conditions of the batch.  It stands
 * directly behind the caller's batch's own 32-bit refusal, ahead of a NULL byte
 * pointer and of a byte that is not above '$': like that refusal it is decided
 * from the offsets, before a byte is read.  The calls without the suffix are the
 * FWD case of these. */
#define GX_STRAND_FWD 1u
#define GX_STRAND_REV 2u
#define GX_STRAND_BOTH 3u
#define GX_STRAND_PAD 16   /* zero bytes staged behind an item batch */
/* dst[j] = strand_comp(src[n - 1 - j]); src and dst do not overlap. */
int  gx_revcomp(const uint8_t* src, size_t n, uint8_t* dst);
/* The item batch exactly as the _strands calls stage it; with a context it is
 * staged on the device (one copy in, the kernel, one copy out).  out_offsets is
 * written first and in full; out_bytes may be NULL (offsets only).  GX_ECAP when
 * the item bytes exceed out_cap: out_bytes untouched.  When out_cap has room for
 * GX_STRAND_PAD bytes more, the zero bytes staged behind the items are written
 * too.  Bytes are refused as the searches refuse them (above '$'). */
int  gx_revcomp_batch(gx_context* ctx /* NULL: host */, const uint8_t* bytes, const uint64_t* offsets /* n+1 */, size_t n,
                      uint32_t strands, uint8_t* out_bytes, size_t out_cap, uint64_t* out_offsets /* items+1 */);
int  gx_suffix_index_search_strands(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets /* npat+1 */,
                                    size_t npat, uint32_t strands, gx_search_hit* hits /* items */, uint32_t max_hits,
                                    uint32_t* positions, size_t positions_cap, uint64_t* hit_offsets /* items+1 */);
int  gx_suffix_index_search_approx_strands(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets,
                                           size_t npat, uint32_t strands, uint32_t k, gx_approx_hit* hits, uint32_t max_hits,
                                           uint32_t* positions, uint8_t* distances, size_t positions_cap,
                                           uint64_t* hit_offsets);
int  gx_suffix_index_search_edit_strands(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets, size_t npat,
                                         uint32_t strands, uint32_t k, gx_edit_hit* hits, uint32_t max_hits, uint32_t* ends,
                                         uint8_t* distances, uint32_t* starts, size_t positions_cap, uint64_t* hit_offsets);
int  gx_suffix_index_extend_strands(gx_suffix_index* idx, const uint8_t* patterns, const uint64_t* offsets, size_t npat,
                                    uint32_t strands, const uint64_t* hit_offsets /* items+1 */, const uint32_t* starts,
                                    const uint32_t* ends, const gx_scores* scores, uint32_t band, gx_extend_hit* out,
                                    uint32_t* cigar, size_t cigar_cap, uint64_t* cigar_offsets);
int  gx_suffix_index_match_stats_strands(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets, size_t nq,
                                         uint32_t strands, uint32_t max_len, gx_match_stat* stats /* item bytes */);
int  gx_suffix_index_mems_strands(gx_suffix_index* idx, const uint8_t* queries, const uint64_t* offsets, size_t nq,
                                  uint32_t strands, uint32_t min_len, gx_mem* mems, size_t mems_cap,
                                  uint64_t* mem_offsets /* items+1 */, uint64_t* candidates /* items */);
/* The last search-mode call on ctx: the items it staged, the reverse bytes the
 * kernel wrote (0: forward only) and that kernel's device time (ms).
 * Measurement and tests. */
int  gx_strand_info(const gx_context* ctx, uint64_t* items, uint64_t* rc_bytes, double* rc_ms);

#ifdef __cplusplus
}
#endif

#endif /* GX_H */
