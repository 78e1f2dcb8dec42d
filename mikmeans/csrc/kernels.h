// mikmeans — host-side launcher declarations for the gfx950 kernels.
//
// Every launcher is stream-ordered (takes the hipStream_t it must launch on),
// allocates nothing and never synchronises, so a caller may capture a whole
// Lloyd iteration into a hipGraph.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispatch.h"   // for_width: the (dtype, padded width) switch of every launcher that has one
#include "fold.h"       // the frame constants of the per-cluster folds (FOLD_*)
#include "pqplan.h"     // the launch planning of the product-quantised scan (PQ_*, pq_scan_splits)
#include "rerankplan.h" // the launch planning of the re-rank kernel (RR_*, rr_run)
#include "walk.h"       // the work item of a walk over an index's lists, its grid bound, walk_blocks

namespace mk {

enum DType : int { DT_F32 = 0, DT_BF16 = 1 };
static_assert(DT_BF16 == WIDTH_BF16, "dispatch.h for_width takes these dtype codes");

// Number of f64 accumulation slots the assign kernel spreads its per-workgroup
// inertia / changed-label partials over (slot = blockIdx % NSLOT, 8 doubles each).
constexpr int NSLOT = 256;
constexpr int SLOT_STRIDE = 8;

// ---- centroid packing -------------------------------------------------------
// The assign kernel reads centroids from a "fragment-packed" array: for tile t (16
// centroids) and 16-byte piece q, the 64 lanes' MFMA A-operand fragments are stored
// contiguously (1 KiB), so one LDS-DMA wave-instruction stages a piece and one
// ds_read_b128 per lane fetches it conflict-free.
//   element (k, d): t = k/16, r = k%16, q = d / (4V), g = (d / V) % 4
//   offset = ((t*NQ + q)*64 + r + 16*g)*V + d%V,  V = 16/sizeof(T), NQ = DPAD/(4V)
// (piece q of lane group g holds features [(4q+g)V, +V): the four lane groups of a
// point read 64 contiguous bytes of its row per fragment load, see assign16.hip)
// The stored value is -2*c (exact in bf16/f32) and cn[k] = |c_q|^2 of the quantised
// centroid, so the MFMA chain seeded with cn directly yields
// score = |c|^2 - 2 x.c  (= |x-c|^2 - |x|^2).
// A/B experiment switches (scripts/ab_ext.py, A/B harnesses, tests).  No launcher reads the
// environment: the values are taken from MIKMEANS_<NAME> once when the extension loads and
// changed only through set_variant (mikmeans.ops.native.variant); -1 = the built-in rule.
// A captured hipGraph keeps the geometry that was in force when it was recorded.
// (Round 6 removed the measured losers: the persistent grid with a second fragment set, the
// centre-stationary kernel, the first-wave stagger and the prologue priority; their results
// stay in profiles/.)
// V_ASSIGN_PERSIST: 0 = the one-pass grid, 1 = the persistent kernel wherever it applies (plain
// full bf16 D=128 passes with caller norms), n >= 2 = on a grid of n workgroups (tests).
enum Variant { V_ASSIGN_VARG = 0, V_ASSIGN_PMAJ, V_ASSIGN_GEOM, V_UPDATE_KS, V_UPDATE_KS_GM, V_BLOBS_TPR,
               V_ASSIGN_TOP2_GEOM, V_ASSIGN_EPI, V_ASSIGN_EARLY, V_COLSTAT_BLOCKS, V_ASSIGN_PERSIST, V_COUNT };
int variant(Variant v);
void set_variant(Variant v, int value);

int assign16_chunk_tiles(int dtype, int dpad);  // centroid tiles per LDS chunk (0 = unsupported)
int assign_kpad(int dtype, int dpad, int K);     // K rounded to a chunk multiple
int assign_cn_len(int kpad);                     // cn array length (multiple of 256 floats)

struct AssignArgs {
  const void* X; int64_t N; int D; int64_t ldx;
  const void* Cpack; const float* cn; int Kpad;
  const float* xn;      // optional: |x|^2 per row, needed for mind/inertia
  int32_t* labels;      // in/out (old labels read when track_changed)
  float* mind;          // optional: squared distance to the chosen centroid
  double* slots;        // optional: [NSLOT][SLOT_STRIDE] order-free digit slots (common.h slot_add)
  int track_changed;
  // optional u64 [N] all-ones scratch; small N then splits the centre range over
  // grid.y (split_finish_kernel writes labels and restores the all-ones)
  unsigned long long* split_keys = nullptr;
  // optional gathered batch: logical row i is X row rows[i] (labels / mind / xn stay
  // logical; without xn the inertia uses |x|^2 of the gathered fragments)
  const int64_t* rows = nullptr;
  // bounded E-step (models/lloyd.py, Hamerly bounds): with ub/lb the kernel also tracks each
  // point's second-smallest score and writes ub = distance to the chosen centre, lb = distance
  // to the second nearest (one-pass grid, no value-only argmin); scatter: a gathered batch's
  // outputs (labels, mind, ub, lb) and inputs (old labels, xn) live at row rows[i], not at i
  float* ub = nullptr;
  float* lb = nullptr;
  int scatter = 0;
  // optional device row count (int64): the launch covers N rows, the kernel assigns the first
  // min(N, *n_dev) -- a compacted batch whose size only the device knows (no host sync, so
  // the bounded E-step captures into a graph); workgroups past it exit at once
  const int64_t* n_dev = nullptr;
  // optional per-row seed offsets (bf16, indexed by X row): every row's scores are seeded with
  // oseed[row] -- the offset the full (ungathered) pass gives it, from launch_seed_offsets -- so a
  // gathered batch ranks each row bitwise as the full pass does (the bounded E-step)
  const float* oseed = nullptr;
  // optional timeline (profiling, launcher-set from set_assign_timeline): per workgroup 8 u64 --
  // real-time ticks (10 ns) at entry, chunk-loop start, epilogue start and exit, then HW_ID
  // and XCC_ID (which CU ran it), then the tick wave 0's prologue loads had all landed
  unsigned long long* timeline = nullptr;
  // launcher-set (A/B switch V_ASSIGN_EPI, default on): the epilogue's old labels and caller
  // norms are fetched with the prologue's fragments instead of in the epilogue
  int epi_prefetch = 1;
  // launcher-set (A/B switch V_ASSIGN_EARLY): norms first, fragments in flight across the
  // seed-offset barrier (plain full bf16 rows with caller norms)
  int early_prologue = 1;
  // optional per-group seed statistics of a plain full pass (launch_group_norm_stats over this call's xn,
  // f32 pairs): group g's (max, min) |x|^2 -- the bf16 kernels whose workgroup is GSTATS_ROWS rows read their
  // seed decision from it instead of reducing the norms (early prologue, persistent kernel); the values,
  // and so every key, are the same.  nullptr, or any other path: the kernel's own reduction.
  const float* gstats = nullptr;
};
// (max, min) of xn over each GSTATS_ROWS-row group of the one-pass grid, the last over its valid rows: the
// folds of the assign's seed rule (fmaxf from 0, fminf from 3e38).  X and so xn are fixed for a fit: once
// per fit.  row0: the global row of xn[0], which must lie on the group grid (ROW_ALIGN shards do).
constexpr int GSTATS_ROWS = 256;
hipError_t launch_group_norm_stats(const float* xn, int64_t n, int64_t row0, float* out, hipStream_t s);
// Profiling hook: every assign16 launch writes its workgroups' timelines to buf (nullptr: off;
// the caller sizes it for the grid, 8 u64 per workgroup, capacity in workgroups)
void set_assign_timeline(unsigned long long* buf, int64_t capacity);
hipError_t launch_assign16(int dtype, int dpad, const AssignArgs& a, hipStream_t s);
// Rows per workgroup of the full (ungathered, unbounded) assign for this shape: the block its
// bf16 seed offset is taken over (the workgroup of the geometry launch_assign16 picks: both
// read it off assign_geometry in csrc/assign16.hip)
int assign16_block_rows(int dtype, int dpad, int kpad);
// oseed[i] = the full pass's seed offset of row i (block_rows from assign16_block_rows; bf16)
hipError_t launch_seed_offsets(const float* xn, int64_t n, int block_rows, float* oseed, hipStream_t s);

// ---- transform: every row's distance to every centre (csrc/transform.hip) --------------
struct TransformArgs {
  const void* X; int64_t N; int D; int64_t ldx;
  const void* pack; const float* cn; int K; int Kpad;   // the assign kernel's packed centres
  const float* xn;      // |x|^2 per row
  float* out; int64_t ldo;
  int squared;          // 1: squared distances, 0: distances
};
hipError_t launch_transform(int dtype, int dpad, const TransformArgs& a, hipStream_t s);

// ---- top-m: every row's m nearest centres (csrc/topk.hip) -------------------------------
// dist[i, j], idx[i, j] = the j-th smallest (squared distance, centre) pair of row i, the
// squared distances bitwise launch_transform's, ties to the lower centre index; 1 <= m <= min(K, TOPK_MAX).
constexpr int TOPK_MAX = 32;
struct TopkArgs {
  const void* X; int64_t N; int D; int64_t ldx;
  const void* pack; const float* cn; int K; int Kpad;   // the assign kernel's packed centres
  const float* xn;      // |x|^2 per row
  float* dist;          // [N, m] squared distances, ascending
  int32_t* idx;         // [N, m] their centres
  int m;
};
hipError_t launch_topk(int dtype, int dpad, const TopkArgs& a, hipStream_t s);

// ---- the clusters as an inverted-file index (csrc/ivf.hip) --------------------------------
// Stable partition by label: order[0..offsets[K]) = the rows i with labels[i] in [0, K), label
// after label and ascending within a label, the tail of order [n] -1; offsets [K + 1] = where each
// label's rows start (the cumulative bincount).  rpos (optional, [n]): every row's position in
// order, -1 for a row in no list.  cells: int64 scratch [K * partition_blocks(n, K)].  Bitwise
// the same on every launch; no host read.  K <= PARTITION_MAX_K (the scatter pass keeps
// [4 waves][K] u32 counters in FOLD_LDS_BYTES of LDS) and n < 2^32.
constexpr int PARTITION_MAX_K = FOLD_LDS_BYTES / 16;   // 10240
int64_t partition_blocks(int64_t n, int K);
hipError_t launch_partition(const int32_t* labels, int64_t n, int K, int64_t* order, int64_t* offsets, int64_t* cells,
                            int64_t* rpos, hipStream_t s);
// Row pack: rows [row0, row0 + nb) of the index (X: the block's rows, in their own dtype) into
// the fragment-packed layout above, list after list, list k from tile toff[k] on (each list
// padded to whole 16-row tiles): row i lands at packed row 16 toff[k] + rpos[i] - offsets[k],
// k = labels[i]; rows with rpos < 0 are skipped.  pack / cn must be filled with zeros /
// PAD_SCORE before the first block.  A list's segment is bitwise launch_finalize's pack-only
// output for its rows.
struct IvfPackArgs {
  const void* X; int64_t nb; int D; int64_t ldx;
  int64_t row0;
  const int32_t* labels;     // [n] every row's list
  const int64_t* rpos;       // [n] launch_partition's
  const int64_t* offsets;    // [K + 1]
  const int64_t* toff;       // [K + 1] first tile of each list
  int K;
  int dtype; int dpad; void* pack; float* cn;
};
hipError_t launch_ivf_pack(const IvfPackArgs& a, hipStream_t s);
// Repack (an index updated in place of a rebuild): the rows that stay move from an old
// (pack, cn) to a new one under new offsets / toff, their bits copied as stored.  The row at
// position p of new list k has the id order[offsets[k] + p]; an id below n_old is an old row and
// comes from old packed row 16 toff_old[k] + rpos_old[id] - offsets_old[k] (rpos_old [n_old]: every
// id's position in the old order, -1 for an id in no list; an id whose old position lies outside
// list k is skipped), an id from n_old on is a new row and is left to launch_ivf_pack.  Out of
// place: the new pack / cn are buffers of their own, filled with zeros / PAD_SCORE by the caller,
// and hold rows_new packed rows (whole tiles); the old ones hold rows_old.
struct IvfRepackArgs {
  const void* pack_old; const float* cn_old; int64_t rows_old;
  const int64_t* offsets_old;   // [K + 1]
  const int64_t* toff_old;      // [K + 1]
  const int64_t* rpos_old;      // [n_old]
  int64_t n_old;
  const int64_t* order;         // [n] the new order
  const int64_t* offsets;       // [K + 1]
  const int64_t* toff;          // [K + 1]
  int64_t n;                    // ids handed out (the length of order)
  int K; int D;
  int dtype; int dpad; void* pack; float* cn; int64_t rows_new;
};
hipError_t launch_ivf_repack(const IvfRepackArgs& a, hipStream_t s);
// A walk over the index's lists (csrc/walk.h), shared by the scan and the range search: the
// (query, probe) pairs -- pair id = query * nprobe + probe -- grouped by probed list (porder / poff:
// launch_partition of the pairs' lists).  A wave's work item is (list, block of up to 16 P pairs
// probing it): icum [K + 1] = the cumulative sum of ceil(pairs_l / 16 P), max_items an upper bound
// of icum[K] (the grid; waves past icum[K] exit), walk_max_items gives one without a host read.
struct IvfWalkArgs {
  const void* Q; int D; int64_t ldq;
  const float* qn;           // |q|^2 per query
  const void* pack; const float* cn;   // the row pack
  const int64_t* offsets;    // [K + 1] list starts in order
  const int64_t* toff;       // [K + 1] list starts in tiles
  const int64_t* order;      // row ids, list after list
  const int64_t* porder;     // [npairs] pair ids grouped by list
  const int64_t* poff;       // [K + 1]
  const int64_t* icum;       // [K + 1]
  int K; int nprobe;
  int64_t npairs; int64_t max_items;
};
// What launch_ivf_scan / launch_ivf_range check of a walk, and its grid: nb = workgroups, 0 where
// there is nothing to do (no pairs); hipErrorInvalidValue for arguments no kernel may see.
hipError_t ivf_walk_grid(const IvfWalkArgs& w, int dpad, int64_t& nb);
// Scan: for every pair of the walk the m smallest keys (d2 bits << 32 | row) over the rows of the
// pair's list, ascending, into out[pair id][0..m); IVF_EMPTY_KEY where the list has fewer than m
// rows.  d2 is bitwise launch_transform's value of the query against the row packed as a centre.
// P from ivf_scan_blocks.  1 <= m <= TOPK_MAX.
constexpr long long IVF_EMPTY_KEY = 0x7fffffffffffffffLL;
struct IvfScanArgs {
  IvfWalkArgs w;
  int m;
  long long* out;            // [npairs, m]
};
int ivf_scan_blocks(int dtype, int dpad, int m, int64_t npairs);
hipError_t launch_ivf_scan(int dtype, int dpad, int P, const IvfScanArgs& a, hipStream_t s);

// ---- range search through the clusters (csrc/range.hip) -----------------------------------
// Every row of a pair's list with bits(d2) <= bits(r2[query]), on the walk's work items (P from
// ivf_range_blocks) and with the scan's d2.  Two launches: the count pass writes counts[pair id]
// (int64), the fill pass writes pair p's keys (d2 bits << 32 | row) in list order from
// keys[base[p]] on -- base = the caller's exclusive cumulative sum of counts in pair-id order,
// total = its end (no key is written at or past it).  r2: one finite non-negative float per
// query.  Bitwise the same on every launch.
struct IvfRangeArgs {
  IvfWalkArgs w;
  const float* r2;           // squared radius per query
  int64_t* counts;           // [npairs] (count pass)
  const int64_t* base;       // [npairs] (fill pass)
  long long* keys;           // [total]  (fill pass)
  int64_t total;
};
int ivf_range_blocks(int dtype, int dpad, int64_t npairs);
hipError_t launch_ivf_range(int dtype, int dpad, int P, bool fill, const IvfRangeArgs& a, hipStream_t s);

// ---- deep search: the m-th smallest d2 of every query by radix select (csrc/deep.hip) -------
// A most-significant-digit radix select over bits(d2) of the rows of a query's probed lists, on
// the walk's work items (P from ivf_hist_blocks) and with the scan's d2: up to four passes of
// 8-bit digits (shift s = 24 - 8 pass), each a histogram over the walk and a select.
// Histogram: every row k < list length of every pair adds one to table[q][bits >> 24] (pass 0) or,
// where bits >> (s + 8) == prefix[q] >> (s + 8), to table[q][(bits >> s) & 255] (passes 1..3).  No
// finiteness filter: an inf or NaN d2 counts (top byte <= 0x7f).  The table (u32 [nq, 256],
// zeroed by the caller) is only ever added into with integer atomics: the same on every launch.
struct IvfHistArgs {
  IvfWalkArgs w;
  int pass;                  // 0..3
  const int32_t* prefix;     // [nq] the bits fixed so far (passes 1..3)
  uint32_t* table;           // [nq, 256]
};
int ivf_hist_blocks(int dtype, int dpad, int64_t npairs);
hipError_t launch_ivf_hist(int dtype, int dpad, int P, const IvfHistArgs& a, hipStream_t s);
// Select, one workgroup a query.  Pass 0: cand[q] = the sum of the bins, R = min(m, cand) - 1;
// later passes R = rank[q].  b = the smallest bin whose running count exceeds R: prefix |= b << s,
// rank = R - the count below b, hits[q] = the rows with bits <= prefix | (2^s - 1), which is
// min(m, cand) - 1 - rank + count[b].  cand = 0: prefix, rank and hits 0.  1 <= m <= IVF_DEEP_MAX_M.
constexpr int IVF_DEEP_MAX_M = 2048;
struct IvfSelectArgs {
  const uint32_t* table;     // [nq, 256]
  int32_t* prefix;           // [nq] in (passes 1..3) / out
  int64_t* rank;             // [nq] in (passes 1..3) / out
  int64_t* hits;             // [nq] out
  int64_t* cand;             // [nq] out (pass 0) / in
  int64_t nq; int m; int pass;
};
hipError_t launch_ivf_select(const IvfSelectArgs& a, hipStream_t s);

// ---- the scan of a product-quantised index (csrc/pq.hip) -----------------------------------
// Pair p = query * nprobe + probe scans list probes[p] of an index whose rows are M-byte codes
// (codes [n, M], the rows of order position after position) against its own table lut[p] [M][256]:
// a row's distance is lut[p][0][c0] + lut[p][1][c1] + ... in that order, float32.  `splits`
// workgroups share a pair (csrc/pqplan.h) and each writes its m smallest keys (sum bits << 32 |
// row), ascending, into out[p][split][0..m); IVF_EMPTY_KEY where it met fewer than m rows.
// M in {8, 16, 32, 64}, 1 <= m <= TOPK_MAX, 1 <= splits <= PQ_MAX_SPLITS; codes and lut 16-byte
// aligned.  Bitwise the same on every launch.
struct PqScanArgs {
  const uint8_t* codes; int64_t n;   // [n, M]
  const int64_t* order;              // [n] row ids, list after list
  const int64_t* offsets;            // [K + 1] list starts in order
  int K; int M;
  const float* lut;                  // [npairs, M, 256]
  const int32_t* probes;             // [npairs] every pair's list
  int64_t npairs;
  int m; int splits;
  long long* out;                    // [npairs, splits, m]
};
static_assert(PQ_MAX_M == TOPK_MAX && PQ_NW == 4, "csrc/pqplan.h mirrors the register-list kernels' constants");
hipError_t launch_pq_scan(const PqScanArgs& a, hipStream_t s);

// ---- the re-rank of candidates against the rows (csrc/rerank.hip) ----------------------------
// out[q][j] = clamp_d2(|Q[q] - X[cand[q][j]]|^2) bits << 32 | cand[q][j] for every candidate id in
// [0, n), IVF_EMPTY_KEY for any other id; an id that appears twice gives its key twice.  The sum is
// the sixteen-accumulator order of docs/PQ_INDEX.md, subtract, multiply and add rounded one by
// one.  Q and X are rows of one dtype with unit column stride and row strides ldq, ldx >= F
// (in elements); pointers or strides off 16 bytes take element loads.  run / runs / items are
// rr_run / rr_runs / rr_items of (nq, R) (csrc/rerankplan.h).  Bitwise the same on every launch.
struct RerankArgs {
  const void* Q; int64_t ldq;        // [nq, F]
  const void* X; int64_t ldx;        // [n, F]
  int64_t n; int F;
  const int64_t* cand;               // [nq, R]
  int64_t nq; int64_t R;
  int run; int64_t runs; int64_t items;
  long long* out;                    // [nq, R]
};
hipError_t launch_rerank(int dtype, const RerankArgs& a, hipStream_t s);

// ---- per-cluster quality table (csrc/quality.hip) ----------------------------------------
// Folds launch_topk's output (m = 1 or 2) into table[K][QUALITY_WORDS] (u64, only ever added
// into) with integer atomics: per label the digits of sum a^2 and the row count, the digits of
// sum a, the non-finite rows, the fixed-point simplified-silhouette sum and the largest a^2.
constexpr int QUALITY_WORDS = 24;
// The LDS-private form (fold.h): words 0..17 of every label in the workgroup's LDS, taken for
// K <= QUALITY_LDS_MAX_K and N >= FOLD_LDS_MIN_ROWS.
constexpr int QUALITY_LDS_WORDS = 18;
constexpr int QUALITY_LDS_MAX_K = FOLD_LDS_BYTES / (QUALITY_LDS_WORDS * 8);   // 1137
struct QualityArgs {
  const int32_t* idx;          // [N, m] centres, nearest first
  const float* dist;           // [N, m] their squared distances
  int64_t N; int m; int K;
  unsigned long long* table;   // [K, QUALITY_WORDS]
};
// path: -1 the rule above (quality_uses_lds), 0 the global-atomic kernel, 1 the LDS-private one.
bool quality_uses_lds(int64_t N, int K);
hipError_t launch_quality(const QualityArgs& a, hipStream_t s, int path = -1);

// ---- per-cluster exemplar table (csrc/exemplars.hip) -------------------------------------
// Min-inserts launch_topk's first column into table[K][m] (u64, all ones = empty, only ever
// min-inserted into): slot j of cluster k is the (j+1)-th smallest key hi << 32 | row of its rows,
// hi = bits(a^2) (nearest) or 0x7F7FFFFF - bits(a^2) (farthest), row = row0 + the row's index.
constexpr int EXEMPLAR_MAX = 64;             // longest list
// The LDS-private form (fold.h): a [K][m] table in the workgroup's LDS; it holds
// K * m <= EXEMPLAR_LDS_MAX_WORDS.  The launcher's rule takes it for
// K * m^2 <= EXEMPLAR_LDS_RULE_KMM and N >= FOLD_LDS_MIN_ROWS: its flush costs every
// workgroup K * m inserts of up to m steps on lists all workgroups share, so it pays for short
// lists and few clusters and loses to the global form beyond (profiles/r7_02_exemplars.md).
constexpr int EXEMPLAR_LDS_MAX_WORDS = FOLD_LDS_BYTES / 8;   // 20480
constexpr int64_t EXEMPLAR_LDS_RULE_KMM = 16384;
struct ExemplarArgs {
  const int32_t* idx;          // [N, mt] centres, nearest first (column 0 is read)
  const float* dist;           // [N, mt] their squared distances
  int64_t N; int mt; int K;
  int m;                       // list length, 1..EXEMPLAR_MAX
  uint32_t row0;               // index of row 0 in the call's X; row0 + N <= 2^32
  int farthest;
  unsigned long long* table;   // [K, m]
};
// path: -1 the rule (exemplar_uses_lds), 0 the global-atomic kernel, 1 the LDS-private one.
bool exemplar_uses_lds(int64_t N, int K, int m);
hipError_t launch_exemplars(const ExemplarArgs& a, hipStream_t s, int path = -1);

// ---- per-cluster distance quantiles (csrc/quantiles.hip) ----------------------------------
// Exact order statistics of every cluster's a^2 = max(dist[i, 0], +0) by a most-significant-
// digit radix select over the distance bits: four passes of 8-bit digits (shift 24, 16, 8, 0),
// each a histogram of launch_topk's first column (u64, only ever added into) and a select that
// fixes one more byte of every (cluster, q) pair's prefix and updates its remaining rank.
constexpr int QUANTILE_MAX_Q = 8;            // most quantiles in one call
constexpr int QUANTILE_BINS = 256;           // one digit
constexpr int QUANTILE_PASSES = 4;
// The LDS-private form (fold.h): a [lists][256] u32 table in the workgroup's LDS;
// lists = K (pass 0) or K * Q (passes 1..3).  A launch takes fewer
// than 2^32 rows, so a u32 bin cannot wrap.  The launcher's rule takes it wherever the lists fit
// and N >= FOLD_LDS_MIN_ROWS: measured (profiles/r7_03_quantiles.md) it is 3 to 200 times
// faster in passes 0 and 1, 0.01 to 0.04 ms slower in passes 2 and 3 on distances without
// ties (where it stays because equal distances put every row of a cluster on one global word),
// and from 8192 rows on never more than 4 us behind.
constexpr int QUANTILE_LDS_MAX_LISTS = FOLD_LDS_BYTES / (QUANTILE_BINS * 4);   // 160
// The banded form: the same kernel for more lists than one workgroup's LDS holds.  Band b (the
// grid's y) keeps lists [160 b, 160 b + 160) in LDS, reads every row and skips the rows of other
// bands: ceil(lists / 160) sweeps over the 8 B rows instead of a global atomic per row.  It
// holds up to QUANTILE_BAND_LIMIT bands.  Measured (profiles/r7_03_quantiles.md, N = 10^7): a
// sweep costs 0.013 ms in pass 0, where the global form's rows meet on one to three words per
// cluster (7 bands 0.10, 26 bands 0.33 against 0.44 ms), and 0.03 to 0.08 ms in pass 1 (3 bands
// 0.19 against 1.0, 8 bands 0.64 against 1.8, 26 bands 0.57 against 0.26 ms); in passes 2 and 3
// few rows match a prefix and the global form (0.03 to 0.3 ms) always wins.  The launcher's
// rule takes it in pass 0 up to QUANTILE_BAND_MAX_PASS0 bands and in pass 1 up to
// QUANTILE_BAND_MAX, from QUANTILE_BAND_MIN_ROWS rows on.
constexpr int QUANTILE_BAND_LIMIT = 64;
constexpr int QUANTILE_BAND_MAX_PASS0 = 26;
constexpr int QUANTILE_BAND_MAX = 8;
constexpr int64_t QUANTILE_BAND_MIN_ROWS = 1 << 18;
// Wave aggregation: up to this many rounds of "the first pending lane's (list, digit) key, a
// ballot of the lanes that share it, one add of their count"; lanes still pending afterwards add
// one each; 0 switches it off.  The global form takes QUANTILE_AGG_ROUNDS, the LDS-private form
// QUANTILE_LDS_AGG_ROUNDS (A/B runs pass their own count).  Measured
// (profiles/r7_03_quantiles.md): on the global form two rounds cost rows in random order under
// 1 % and take pass 0 on rows ordered by label from 0.74 to 0.045 ms (K = 1024), more rounds
// only add to the later passes; LDS atomics on one address need no help, every round there is
// a loss.
constexpr int QUANTILE_AGG_ROUNDS = 2;
constexpr int QUANTILE_LDS_AGG_ROUNDS = 0;
constexpr int QUANTILE_AGG_MAX = 64;
struct QuantileHistArgs {
  const int32_t* idx;          // [N, mt] centres, nearest first (column 0 is read)
  const float* dist;           // [N, mt] their squared distances
  int64_t N; int mt; int K;
  int Q;                       // quantiles, 1..QUANTILE_MAX_Q (pass 0 does not read it)
  int pass;                    // 0..3: the digit at shift 24 - 8 * pass
  const int32_t* prefix;       // [K, Q] the bits fixed so far (passes 1..3)
  unsigned long long* table;   // pass 0: [K, 256]; passes 1..3: [K, Q, 256]
  int agg;                     // wave-aggregation rounds, 0..QUANTILE_AGG_MAX; -1: the form's constant
};
struct QuantileSelectArgs {
  const unsigned long long* table;   // as above, summed over all rows (and ranks)
  const double* q;                   // [Q], each in [0, 1]
  int32_t* prefix;                   // [K, Q] in / out
  int64_t* rank;                     // [K, Q] in (passes 1..3) / out: the rank left below the prefix
  int64_t* counts;                   // [K] out (pass 0): n_k
  int K; int Q; int pass;
};
// path: -1 the rule (quantile_path), 0 the global-atomic kernel, 1 the LDS-private one (the lists
// fit one workgroup), 2 the banded LDS one.
__host__ __device__ inline int64_t quantile_lists(int K, int Q, int pass) { return pass == 0 ? (int64_t)K : (int64_t)K * Q; }
inline int64_t quantile_bands(int64_t lists) { return (lists + QUANTILE_LDS_MAX_LISTS - 1) / QUANTILE_LDS_MAX_LISTS; }
bool quantile_uses_lds(int64_t N, int64_t lists);
int quantile_path(int64_t N, int64_t lists, int pass);
hipError_t launch_quantile_hist(const QuantileHistArgs& a, hipStream_t s, int path = -1);
hipError_t launch_quantile_select(const QuantileSelectArgs& a, hipStream_t s);

// ---- Hamerly bounds (csrc/rows.hip) ----------------------------------------------------
// Moves every point's bounds by the last M-step's centre shifts (ub += |dc_label|,
// lb -= the largest |dc_k| over k != label) and flags the points whose bounds no longer prove
// their label (cand[i] = 1): shift2 = squared shifts [K] of the centres the assign ranks
// (finalize qshift); cn = |c|^2 of the packed centres, xn = |x|^2, oseed (bf16: the rows'
// full-pass seed offsets, else null) and nterms (the features) size the rounding slack of the
// kernel's scores; work: 4 floats scratch.  A row stays unflagged only where the full
// assign's keys provably keep its label (the slack counted on both sides of the test), so
// skipping it changes nothing.
hipError_t launch_bounds_update(const int32_t* labels, float* ub, float* lb, const float* shift2, const float* cn,
                                int K, const float* xn, int64_t n, uint8_t* cand, float* work, const float* oseed,
                                int nterms, hipStream_t s);
// rows[0..*count) = indices of the nonzero flags, ascending (deterministic, no host sync);
// bscratch: int64 [compact_blocks(n)]
int64_t compact_blocks(int64_t n);
// Hamerly's tightening over the compacted candidates rows[0..*count): ub = |x - c_label| (f32
// centres C [K][ldc], bf16-rounded for bf16 points: the centres the assign ranks); cand = 0 where the bounds test of launch_bounds_update passes with it
// (xn, work, oseed as there, nterms = D: work holds that step's slack terms).  n_max bounds *count
hipError_t launch_tighten(int dtype, const void* X, int64_t ldx, int D, const int32_t* labels, const float* C,
                          int64_t ldc, const int64_t* rows, const int64_t* count, int64_t n_max, float* ub,
                          const float* lb, uint8_t* cand, const float* xn, const float* work, const float* oseed,
                          hipStream_t s);
// k-means|| round: cand[i] = u(start + i) < ell * d2[i] / psi[0] (philox uniform keyed by the global row)
hipError_t launch_kpar_select(const float* d2, int64_t n, int64_t start, const double* psi, double ell,
                              uint64_t seed, uint32_t round, uint8_t* cand, hipStream_t s);
hipError_t launch_compact(const uint8_t* cand, int64_t n, int64_t* rows, int64_t* count, int64_t* bscratch,
                          hipStream_t s);

// ---- update (LDS-privatised scatter-add) -------------------------------------
// Sums are accumulated in FIXED POINT: every contribution x*w is rounded to a
// 32-bit integer at scale 2^sum_exp (|x*w| * 2^sum_exp <= 2^30) and added with
// 64-bit integer LDS atomics (ds_add_u64, ~8 cycles per wave-instruction on
// gfx950, against ~170 for ds_add_f32).  Integer addition is associative, so
// the M-step is bitwise reproducible whatever the atomic order.
struct UpdateArgs {
  const void* X; int64_t N; int D; int64_t ldx;
  const int32_t* labels; int K;
  int n_chunks;          // multiple of 8
  long long* slab;       // [n_chunks][K][D] fixed-point partial sums
  long long* cnt_slab;   // [n_chunks][K] fixed-point partial counts
  const float* weights;  // optional per-row weights (sample_weight)
  const int* col_exp;    // [D] column d's contributions are rne(x * w * 2^col_exp[d]), |.| <= 2^20
  int cnt_exp;           // counts scale 2^cnt_exp (0 when unweighted)
  int clamp;             // saturate contributions outside +-2^20 (streamed data) ...
  int* clamp_count = nullptr;  // ... and count the workgroups that did (optional)
  // Residual (lo) pass of wide-range columns (optional): contributions are
  // rne((x*w*2^col_exp - rne(x*w*2^col_exp)) * 2^(col_exp2 - col_exp)) on columns with
  // col_exp2 > -200, nothing elsewhere; slices without such a column are skipped.
  const int* col_exp2 = nullptr;
  // Incremental M-step (optional): rows whose label changed since the last M-step, as
  // (row, previous label) pairs from launch_label_delta.  Each is added to its new
  // label and subtracted from its old one; when *dcount > dcap the list overflowed
  // and the kernel accumulates all N rows instead (the reduce then restarts totals).
  const int2* dlist = nullptr;
  const int* dcount = nullptr;
  int dcap = 0;
  // Gathered batch (optional, plain passes only): logical row i is X row rows[i], so a
  // mini-batch drawn from an HBM-resident shard is never copied (labels / weights logical).
  const int64_t* rows = nullptr;
};
int update_slice_width(int dtype, int K, int D, bool weighted = false);  // 0 = global fallback
int update_n_chunks(int dtype, int K, int D, int64_t N, bool weighted = false);
int fixed_exp(double maxabs);                     // largest e with maxabs * 2^e <= 2^20
void set_update_max_sw(int sw);                   // cap the slice width (0 = none)
hipError_t launch_update(int dtype, const UpdateArgs& a, hipStream_t s);
// Changed rows: for every i with labels[i] != prev[i], append (i, prev[i]) to list
// (first `cap` entries kept, *count counts all) and set prev[i] = labels[i].
// Zeroes *count first (stream-ordered).
hipError_t launch_label_delta(const int32_t* labels, int32_t* prev, int64_t N, int2* list, int cap,
                              int* count, hipStream_t s);
// The same over the candidate rows rows[0..*rcount) only (bounded E-step; n_max >= *rcount)
hipError_t launch_label_delta_rows(const int32_t* labels, int32_t* prev, const int64_t* rows, const int64_t* rcount,
                                   int64_t n_max, int2* list, int cap, int* count, hipStream_t s);

// Reduce slabs (+ assign slots) into the packed f64 message
// [K*D sums | K counts | inertia | n_changed] (length K*D + K + 2).
hipError_t launch_reduce(const long long* slab, const long long* cnt_slab, int n_chunks, int K,
                         int D, const int* col_exp, int cnt_exp, double* slots, double* packed,
                         hipStream_t s, long long* tot = nullptr, const int* dcount = nullptr,
                         int dcap = 0);
// With `tot` ([K*D + K] int64, persistent across iterations): tot += slab sums (or
// tot = slab sums when *dcount > dcap), and the message is built from tot.
// out[k*nw + j] = 2^-exps[j] * sum_c slab[c][k][cols[j]]  (wide-column lo sums)
hipError_t launch_reduce_cols(const long long* slab, int n_chunks, int K, int D, const int* cols,
                              const int* exps, int nw, double* out, hipStream_t s);

// ---- finalize (new centroids + shift + re-pack) -------------------------------
enum FinalizeMode : int { FIN_PACK_ONLY = 0, FIN_LLOYD = 1, FIN_MINIBATCH = 2 };
struct FinalizeArgs {
  const double* packed;   // may be null for FIN_PACK_ONLY
  const float* Cold; float* Cnew; int K; int D;
  const uint8_t* frozen;  // optional
  double* mb_counts;      // FIN_MINIBATCH running per-centre counts
  int dtype; int dpad; int Kpad;
  void* pack; float* cn;
  float* shift;           // optional [K]
  float* counts_out;      // optional [K]
  int mode;
  // optional [K]: |q(C_new) - q(C_old)|^2, the move of the quantised centres the assign ranks
  // (q = bf16 rounding; the f32 shift for f32 points) -- the bounded E-step's shifts
  float* qshift = nullptr;
};
hipError_t launch_finalize(const FinalizeArgs& a, hipStream_t s);

// ---- row squared norms -------------------------------------------------------
// Per-column max |x| (as f32 bit patterns, atomicMax into a zeroed out[D]); optionally, all
// together, fstats = [sum |x| | sum x | sum x^2] (f64 [3][D], zeroed), the nonzero count
// (u64 [D], zeroed) and the lowest set bit's exponent over nonzero finite values (int [D],
// initialised to INT_MAX by the caller).
// The f64 sums are bitwise reproducible: each block writes its partials to its row of fpart
// (f64 [colstat_rows(dtype, N, D)][3][D], zeroed by the caller) and one fixed-order pass sums them.
// xn (optional, D <= 64 pieces): every row's |x|^2 from the same pass, bitwise row_sqnorm's.
int colstat_blocks();
int colstat_rows(int dtype, int64_t N, int D);   // fpart rows one launch_col_absmax call writes
hipError_t launch_col_absmax(int dtype, const void* X, int64_t N, int D, int64_t ldx, uint32_t* out,
                             hipStream_t s, double* fstats = nullptr, unsigned long long* nnz = nullptr,
                             int* lowbit = nullptr, double* fpart = nullptr, float* xn = nullptr);
hipError_t launch_row_sqnorm(int dtype, const void* X, int64_t N, int D, int64_t ldx, float* out,
                             hipStream_t s);

// ---- rows (csrc/rows.hip) ----------------------------------------------------------
// Mini-batch sampler: out[j] = X[idx_j] for j < b, idx_j = floor(u * n) from Philox keyed by
// (seed; j, step, rank) (NumPy mirror: mikmeans/data/sampler.py); xn / idx_out optional.
hipError_t launch_sample_rows(int dtype, const void* X, int64_t n, int64_t ldx, int D, void* out,
                              int64_t ldo, int64_t b, uint64_t seed, uint32_t rank, uint32_t step,
                              float* xn, int64_t* idx_out, hipStream_t s);
// idx[j] = the sampler's source row of batch row j (the same draws as launch_sample_rows).
hipError_t launch_sample_index(int64_t n, int64_t b, uint64_t seed, uint32_t rank, uint32_t step, int64_t* idx,
                               hipStream_t s);
// In place x <- x / max(|x|, 1e-30) per row (cosine metric); xn (optional) = |x_rounded|^2.
hipError_t launch_row_normalize(int dtype, void* X, int64_t N, int D, int64_t ldx, float* xn, hipStream_t s);
// out[0] += sum a[i] * b[i] (f64 accumulation, deterministic order; scratch: wdot_scratch_len() f64).
int wdot_scratch_len();
hipError_t launch_wdot(const float* a, const float* b, int64_t n, double* out, double* scratch, hipStream_t s);

// ---- k-means++ ---------------------------------------------------------------
// With owner[N] (int32: centre each d2 was measured against) and cc[k] (|c - c_j|^2, from
// launch_kpp_cc) rows the triangle inequality rules out are not read (bit-identical
// result); knew >= 0 records the new centre as the owner of rows whose d2 drops.
// The new centre is staged in LDS, so rows have at most KPP_MAX_D (padded) columns.
constexpr int KPP_MAX_D = 16376;
hipError_t launch_kpp_d2(int dtype, const void* X, int64_t N, int D, int64_t ldx, const float* c,
                         int first, float* d2, double* block_sums, int64_t rows_per_block,
                         int nblocks, hipStream_t s, int32_t* owner = nullptr,
                         const float* cc = nullptr, int kcc = 0, int knew = -1);
hipError_t launch_kpp_cc(const float* C, int64_t ldc, int k, int D, const float* cnew, float* cc,
                         hipStream_t s);
// mode 0: target = device double (rank-local; < 0 writes zeros to crow); mode 1: target
// holds u, scaled by this rank's total; mode 2: target holds u, totals_all[world] decide
// the owner rank and its local target on device.
hipError_t launch_kpp_sample(int dtype, const double* block_sums, int nblocks, const float* d2,
                             int64_t N, int64_t rows_per_block, const double* target, const void* X,
                             int D, int64_t ldx, float* crow, int64_t* idx_out, int mode,
                             const double* totals_all, int world, int rank, hipStream_t s);

// Weighted k-means++ over M candidates (the k-means|| recluster): Ct f32 [D][M] (column-major),
// w f64 [M], u f64 [K]; d2 f64 [M] (= +inf before the first step), cum f64 [M] and part f64
// [ceil(M/256)] scratch, state int64 {previous pick (-1 first), next k}.  Enqueues `steps`
// draws, each writing out[k][0..D) (row stride ldo); no host read.
hipError_t launch_wkpp(const float* Ct, int64_t M, int D, const double* w, double* d2, double* cum, double* part,
                       const double* u, int64_t* state, float* out, int64_t ldo, int steps, hipStream_t s);

// ---- synthetic Gaussian blobs (counter-based Philox, deterministic by index) --
hipError_t launch_blob_centers(float* centers, int n_centers, int D, float box, uint64_t seed,
                               hipStream_t s);
hipError_t launch_blobs(int dtype, void* X, int64_t i0, int64_t n, int D, int64_t ldx,
                        const float* centers, int n_centers, float stddev, uint64_t seed,
                        int32_t* y, float* xn, hipStream_t s);

}  // namespace mk
