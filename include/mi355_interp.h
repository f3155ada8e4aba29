/*
 * mi355_interp.h -- C ABI of libmi355interp.so, the MI355X (gfx950) native
 * batched linear-interpolation path.
 *
 * This is the drop-in boundary for the hot path of
 * kyle-wedgwood/ArmadilloCUDALinearInterpolation.  The reference has no FFI of
 * its own (it is one nvcc-built C++ program); what it has is
 *   - the operator interface  AbstractNonlinearProblem::ComputeF(const
 *     arma::vec&, arma::vec&)           (AbstractNonlinearProblem.hpp:11), and
 *   - the device stages that EventDrivenMap::ComputeF launches
 *     (EventDrivenMap.cu:154-240).
 * Every entry point below names the reference code it replaces.  The
 * Armadillo-facing C++ signatures that sit on top of this ABI are in
 * include/mi355_arma.hpp; the binding a reference maintainer would add is
 * shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; every function returns an mi_status (0 = MI_OK) and
 *     never calls exit() (the reference's CUDA_CALL macros do,
 *     EventDrivenMap.cu:18-54; the C++ wrapper restores that behaviour).
 *   - mi_last_error(ctx) returns the message of the last failure on that
 *     context (or on the calling thread when ctx is NULL).
 *   - a context is not thread-safe (one host thread per context, like the
 *     reference's single-threaded driver); use one context per thread/stream.
 *   - "dev" pointers are HBM addresses valid on the context's device; "host"
 *     pointers are ordinary host memory.  Device entry points are
 *     asynchronous on the context's stream and perform no allocation, copy or
 *     synchronisation (safe to capture into a hipGraph).
 *   - fp64 blend shared by every interp entry point (Armadillo
 *     interp1_helper_linear semantics, see oracle/interp_oracle.c):
 *        l = largest node with X[l] <= q,  r = min(l+1, n-1)
 *        a = q - X[l];  b = X[r] - q;  w = a > 0 ? a/(a+b) : 0
 *        out = (1-w)*Y[l] + w*Y[r]          (every op rounded, no FMA)
 *     q < X[0] or q > X[n-1] -> extrap_val;  q = NaN -> NaN.
 *   - nearest rule shared by every "nearest" entry point (arma::interp1's
 *     "nearest" / "*nearest", interp1_helper_nearest):
 *        q = NaN                   -> NaN
 *        q < X[0] or q > X[n-1]    -> extrap_val
 *        otherwise   l = largest node with X[l] <= q,  r = min(l+1, n-1)      (the blend's bracket)
 *                    a = q - X[l];  b = X[r] - q        (one rounded fp64 subtraction each)
 *                    k = (b < a) ? r : l                (a tie keeps the LEFT node)
 *                    out = Y[k]                          (a copy: no arithmetic touches the value)
 *     inf, -0.0, denormals and NaN in Y come back exactly as stored, and only for
 *     queries whose nearest node holds them.  The decision comes from a and b
 *     themselves, never from the blend's weight a/(a+b), which rounds and can equal
 *     0.5 when a != b.  Armadillo scans the nodes and stops at the first error that
 *     does not decrease (err >= best_err), which also keeps the left node of a tie;
 *     the rule equals that scan whenever fl(|X[j]-q|) strictly decreases along it.
 *     The one deviation: where two nodes in front of the nearest one are so close
 *     that their rounded distances to q are equal (X = [0, 2^-60, 1, 2], q = 1:
 *     1 - 0 and 1 - 2^-60 round to the same double) the scan stops there (node 0)
 *     and the rule returns the true nearest node (node 2).  DESIGN.md section 2.
 *   - 2-D nearest rule shared by every interp2 "nearest" entry point (arma::interp2's
 *     "nearest" is separable: interp2_helper_nearest along one axis, then along the
 *     other, so the 1-D rule per axis is the 2-D rule):
 *        kx = nearest-rule node of XI[j] on the x axis     (the 1-D rule, unchanged: bracket l, r = min(l+1, n-1),
 *        ky = nearest-rule node of YI[i] on the y axis      a = q - X[l], b = X[r] - q, k = (b < a) ? r : l; a tie keeps the LEFT node)
 *        either coordinate NaN                 -> NaN                      (NaN wins over out-of-range)
 *        else either coordinate out of range   -> extrap_val
 *        else                                  -> Z(ky, kx), the stored 64 bits: inf, NaN, -0.0 and denormals as they are
 *     A special value in Z reaches exactly the outputs whose (ky, kx) is its node.
 *     XI and YI may be in any order (Armadillo demands ascending order; the linear
 *     calls here do not, and neither do these).
 */
#ifndef MI355_INTERP_H
#define MI355_INTERP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (round 3): + mi_group_rccl_ranks, mi_ctx_set_interp2_path, mi_grid2_reserve, mi_grid2_info;
 *              - mi_debug_sweep_timing (the sweep's phase stamps live in scripts/ harnesses now)
 * 4 (round 4): - mi_ctx_set_interp2_path, mi_grid2_reserve, MI_INTERP2_* (the call-wide cell ordering of the bilinear path
 *                was bit-identical and 24 % slower than the direct kernel; it is a recorded experiment now,
 *                scripts/exp_interp2_ordered.hpp, profiles/r03_config3_ordered_*); mi_grid2_info reports the table size only;
 *              + mi_edm_set_kernel_choice (replaces two environment hooks), mi_edm_debug_counters,
 *                mi_group_set_gather_chunks;
 *              additive in 4: mi_interp2_grid_f64_dev, mi_interp2_grid_f64_host, mi_group_interp2_grid_f64_host (the
 *                gridded arma::interp2 output); mi_axis1_create, mi_axis1_create_uniform, mi_axis1_destroy,
 *                mi_interp1_cols_f64_dev, mi_interp1_cols_f64_host, mi_group_interp1_cols_f64_host (interp1 over the
 *                columns of a matrix: one X, many Y); mi_interp1_pairs_f64_dev, mi_interp1_pairs_f64_host,
 *                mi_group_interp1_pairs_f64_host (interp1 over paired columns: every column of Y with its own X);
 *                mi_interp1_each_f64_dev, mi_interp1_each_f64_host, mi_group_interp1_each_f64_host,
 *                mi_debug_each_launches (paired columns with a query vector per column, and a thin kernel for very
 *                short columns); mi_interp2_slices_f64_dev, mi_debug_slices2_launches (gridded interp2 over the slices of a
 *                cube, Z read in place; device form); mi_interp1_rows_f64_dev, mi_debug_rows1_launches (interp1 along
 *                the rows of a matrix / across the slices of a cube: one X, a table per row; device form only);
 *                mi_interp1_rowpairs_f64_dev, mi_debug_rowpairs_launches (interp1 over paired rows: every row of Y with
 *                its own X, realisation-fastest data; device form only);
 *                mi_group_wait_stream (a group member's stream behind a stream of the caller's);
 *                mi_interp1_nearest_f64_dev, mi_interp1_nearest_f64_host, mi_interp1_nearest_f64,
 *                mi_interp1_cols_nearest_f64_dev, mi_debug_nearest_launches (arma::interp1's "nearest" method: table
 *                lookup on the mi_grid1 handles of the linear calls, and the columns of a matrix; device form only
 *                for the columns);
 *                mi_interp1_rows_nearest_f64_dev, mi_interp1_pairs_nearest_f64_dev, mi_debug_nearest_batched_launches
 *                (the "nearest" method along the rows of a matrix / across the slices of a cube, and over paired
 *                columns; device form only);
 *                mi_interp1_f64_dev_v2_base, mi_debug_sweep_ds_launches_base, mi_debug_interp1_phased_sweep (the region
 *                sweep with the XCD groups out of phase, csrc/mi_sweep_phase.hip: the interp1 family's own dispatcher
 *                and counter under a second name, and the phased kernel on its own for tests);
 *                mi_debug_interp1_phased_sweep_ex, mi_debug_sweep_partition (the phase classes set apart by work
 *                instead of a clock wait: the kernel on its own with a first-tile table and optional clock stamps,
 *                and the ownership function, csrc/mi_sweep_partition.hpp, on the host);
 *                mi_interp2_nearest_f64_dev, mi_interp2_grid_nearest_f64_dev, mi_interp2_grid_nearest_f64_host,
 *                mi_interp2_slices_nearest_f64_dev, mi_debug_nearest2_launches (arma::interp2's "nearest" method:
 *                scattered pairs and the gridded output on a mi_grid2, and the gridded output over the slices of a cube) */
#define MI355_INTERP_ABI_VERSION 4

typedef int mi_status;
enum {
    MI_OK = 0,
    MI_ERR_INVALID_ARG = 1,   /* NULL pointer, bad size, bad flag               */
    MI_ERR_GRID = 2,          /* grid not sorted/unique, NaN node, < 2 nodes    */
    MI_ERR_HIP = 3,           /* a HIP runtime call failed (message has detail) */
    MI_ERR_NOMEM = 4,
    MI_ERR_NO_DEVICE = 5
};

typedef struct mi_ctx mi_ctx;       /* one per device (+ stream)            */
typedef struct mi_grid1 mi_grid1;   /* HBM-resident 1-D table               */
typedef struct mi_grid2 mi_grid2;   /* HBM-resident 2-D table               */
typedef struct mi_axis1 mi_axis1;   /* validated 1-D axis (nodes only)      */
typedef struct mi_edm mi_edm;       /* EventDrivenMap device state          */
typedef struct mi_timer mi_timer;   /* pair of HIP events on the ctx stream */

/* ---- context ---------------------------------------------------------- */
/* Replaces the implicit "device 0, NULL stream" of the reference
 * (EventDrivenMap.cu:80-94 allocates on the current device). */
mi_status mi_ctx_create(int device, mi_ctx** out);
mi_status mi_ctx_destroy(mi_ctx* ctx);
/* stream: a hipStream_t (NULL = the device's default stream). */
mi_status mi_ctx_set_stream(mi_ctx* ctx, void* stream);
/* give the context a non-blocking stream of its own (created here, destroyed with the context): lets work of
 * several contexts on one device overlap without the caller touching the HIP API */
mi_status mi_ctx_own_stream(mi_ctx* ctx);
mi_status mi_ctx_synchronize(mi_ctx* ctx);
const char* mi_last_error(const mi_ctx* ctx);
int mi_abi_version(void);
/* Test hook: number of caller host ranges the library currently keeps page-locked on behalf of host-convenience calls
 * in flight (mi_interp1_f64_host, mi_interp2_f64_host); 0 once every such call has returned, on success or error. */
size_t mi_debug_pinned_ranges(void);
/* Test hook: launches of the deferred-store region sweep (mi_interp1_f64_dev_v2) by this process so far. */
size_t mi_debug_sweep_ds_launches(void);
/* Test hook: the part of mi_debug_sweep_ds_launches that the interp1 family's own deferred-store kernel accounts for
 * (csrc/mi_interp1.hip); the rest are launches of the phased kernel (csrc/mi_sweep_phase.hip). */
size_t mi_debug_sweep_ds_launches_base(void);
/* Test hook: calls of mi_interp1_each_f64_dev by this process so far that took the given form: 0 thin kernel, 1 LDS
 * form, 2 direct form, 3 forwarded to mi_interp1_pairs_f64_dev; 0 for any other value of form. */
size_t mi_debug_each_launches(int form);
/* Test hook: calls of mi_interp2_slices_f64_dev by this process so far that took the given form: 0 LDS form with the
 * tile body, 1 LDS form with the flat body (thin outputs, nyi < 256), 2 direct form with the tile body, 3 direct form
 * with the flat body; 0 for any other value of form. */
size_t mi_debug_slices2_launches(int form);
/* Test hook: calls of mi_interp1_rows_f64_dev by this process so far that took the given form: 0 tile body with 16-B
 * accesses, 1 tile body with 8-B accesses, 2 flat body (m < 256); 0 for any other value of form. */
size_t mi_debug_rows1_launches(int form);
/* Test hook: calls of mi_interp1_rowpairs_f64_dev by this process so far that took the given form: 0 short-row form
 * (n <= 32, one launch), 1 long-row form (validation pass, then the march); 0 for any other value of form. */
size_t mi_debug_rowpairs_launches(int form);
/* Test hook: calls of the nearest entry points by this process so far that took the given form: 0 streaming kernel,
 * 1 whole table in LDS, 2 scalar kernel (pointers not 16-B aligned) -- mi_interp1_nearest_f64_dev; 3 columns LDS form,
 * 4 columns direct form -- mi_interp1_cols_nearest_f64_dev; 0 for any other value of form. */
size_t mi_debug_nearest_launches(int form);
/* Test hook: calls of the batched nearest entry points by this process so far that took the given form: 0 rows tile body
 * with 16-B accesses, 1 rows tile body with 8-B accesses, 2 rows flat body (m < 256) -- mi_interp1_rows_nearest_f64_dev;
 * 3 pairs LDS form (n <= 4096), 4 pairs direct form -- mi_interp1_pairs_nearest_f64_dev; 0 for any other value of form. */
size_t mi_debug_nearest_batched_launches(int form);
/* Test hook: calls of the interp2 nearest entry points by this process so far that took the given form: 0 scattered --
 * mi_interp2_nearest_f64_dev; 1 tile body with 16-B stores, 2 tile body with 8-B stores, 3 flat body (nyi < 256) with 16-B
 * stores, 4 flat body with 8-B stores -- mi_interp2_grid_nearest_f64_dev (and each chunk of its _host form); 5 tile body
 * with 16-B stores, 6 tile body with 8-B stores, 7 flat body -- mi_interp2_slices_nearest_f64_dev; 0 for any other value. */
size_t mi_debug_nearest2_launches(int form);
/* Test hook: which closed form of the abscissae a mode-0 table evaluates (0 fma(i, dx, x0); 1 x0 + i*dx;
 * 2 x0 + span*(i/(n-1)); 3 the same with the quotient from a Markstein step) and whether its last node is pinned to
 * xmax -- i.e. which instance of the interp1 kernels a call on this table launches.  Both are -1 for the {x,y} modes. */
mi_status mi_debug_grid1_formula(const mi_grid1* g, int* formula, int* pin_last);
/* Hint about the order of the query vectors handed to mi_interp1_f64_dev on this context.  Unordered queries
 * over a table larger than L2 are processed by a "region sweep" kernel (workgroup-local ordering by table region
 * in LDS; results keep the caller's order), ordered/clustered ones by the plain streaming kernel.  AUTO decides on
 * the device with a 1024-sample probe (no host synchronisation): the first call launches both kernels gated on the
 * probe's flag, later calls launch only the kernel the previous probe's verdict predicts (read from a pinned host
 * int, never waited for; both kernels are correct on any input, so a stale verdict only costs time).  The other
 * values skip the probe; changing the value forgets the verdict.  Results never depend on any of this. */
#define MI_QUERIES_AUTO    0
#define MI_QUERIES_RANDOM  1
#define MI_QUERIES_ORDERED 2
mi_status mi_ctx_set_query_order(mi_ctx* ctx, int order);
/* name / CU count of the context's device (for bench reports) */
mi_status mi_ctx_device_info(mi_ctx* ctx, char* name, size_t name_len, int* compute_units,
                             size_t* hbm_bytes);

/* ---- timing (HIP events recorded on the context's stream) -------------- */
mi_status mi_timer_create(mi_ctx* ctx, mi_timer** out);
mi_status mi_timer_destroy(mi_timer* t);
mi_status mi_timer_start(mi_timer* t);
mi_status mi_timer_stop(mi_timer* t);
/* blocks until the stop event has completed */
mi_status mi_timer_elapsed_ms(mi_timer* t, float* ms);

/* ---- 1-D tables ---------------------------------------------------------
 * General grid: explicit abscissae, the arma::interp1(X, Y, XI, YI) shape.
 * x/y are HOST pointers (n doubles each); the table is uploaded once and
 * stays resident in HBM: as Y only when a closed form (linspace-like grids)
 * reproduces every abscissa bit for bit, else as interleaved {x,y} nodes.
 * flags: MI_GRID_SANITISE    sort + de-duplicate X first (what arma::interp1
 *                            does unless the method is "*linear"); without it
 *                            X must be strictly increasing or MI_ERR_GRID.
 *        MI_GRID_DEVICE_PTRS x/y are device pointers (copied to the host once
 *                            for validation and index construction).
 */
#define MI_GRID_SANITISE     0x1u
#define MI_GRID_DEVICE_PTRS  0x2u
mi_status mi_grid1_create(mi_ctx* ctx, const double* x, const double* y, size_t n,
                          unsigned flags, mi_grid1** out);
/* Implicit uniform grid: X_i := fma(i, dx, x0), i = 0..n-1, dx > 0.
 * Only Y is stored (half the table bytes of the general form). */
mi_status mi_grid1_create_uniform(mi_ctx* ctx, double x0, double dx, const double* y, size_t n,
                                  unsigned flags, mi_grid1** out);
mi_status mi_grid1_destroy(mi_grid1* g);
/* number of nodes after sanitising; table mode chosen at build time
 * (0 = Y only, abscissae from a closed form -- declared by
 *      mi_grid1_create_uniform or detected on an explicit grid,
 *  1 = explicit {x,y} nodes + analytic guess and a bounded walk,
 *  2 = explicit {x,y} nodes + bucket index,
 *  3 = explicit {x,y} nodes + centred analytic guess: the grid stays within
 *      one cell of a straight line, the bracket is one comparison away) */
mi_status mi_grid1_info(const mi_grid1* g, size_t* n_nodes, int* mode, size_t* table_bytes);

/* ---- 1-D interpolation: the hot path -----------------------------------
 * yq[i] = interp(grid, xq[i]), i < nq.  Device pointers, asynchronous.
 * Algorithmic HBM bytes per query: 8 (xq) + 8 (yq); the table is read through
 * L2 / Infinity Cache.
 * Generalises RestrictKernel's two-point blend (EventDrivenMap.cu:769-785) to
 * a tabulated grid with a gather index, as BASELINE.json's north_star asks.
 * Kernel choice (launch_mode) and both entry points: csrc/mi_interp1.hip.
 */
mi_status mi_interp1_f64_dev(mi_ctx* ctx, const mi_grid1* g, const double* xq_dev, double* yq_dev,
                             size_t nq, double extrap_val);
/* Same contract, same results bit for bit, same code (csrc/mi_interp1.hip: one dispatcher serves both).  Where
 * mi_interp1_f64_dev runs the pipelined region sweep as its only launch, this runs that kernel with part of each tile's
 * result stores held back and issued beside the next tile's gathers (interp1_sweep_pipe_kernel's DEFER parameter,
 * csrc/mi_interp1_sweep.hpp); every other call does what mi_interp1_f64_dev does.  With MI_SWEEP_DEFER=0 in the
 * environment (read once per process) every call does. */
mi_status mi_interp1_f64_dev_v2(mi_ctx* ctx, const mi_grid1* g, const double* xq_dev, double* yq_dev,
                                size_t nq, double extrap_val);
/* mi_interp1_f64_dev_v2 is defined in csrc/mi_sweep_phase.hip: exactly where the dispatcher above would launch the
 * deferred-store sweep of a closed-form table (mode 0) as the call's only kernel, it launches that kernel's restatement
 * with the XCD groups out of phase (same results bit for bit); every other call, argument errors included, goes to
 * mi_interp1_f64_dev_v2_base, which is csrc/mi_interp1.hip's dispatcher as it is.
 * MI_SWEEP_XCD_PHASES=P[:period_ns[:units]] in the environment (read once per process) sets the number of phase classes
 * (1, 2, 4, 8), the tile period the clock delays are cut from, and the first-tile table of the shift by work, a digit
 * 1..4 per class ("4:0:4123"; P = 1, 2, 4 only).  Without a units field, period_ns > 0 asks for the clock form and
 * anything else runs the form shipped for P.  P = 0, or any of the family's MI_SWEEP_* hooks present, forwards every
 * call to the base. */
mi_status mi_interp1_f64_dev_v2_base(mi_ctx* ctx, const mi_grid1* g, const double* xq_dev, double* yq_dev,
                                     size_t nq, double extrap_val);
/* Test hook: the phased kernel on its own, whatever the size thresholds say, on at most max_workgroups workgroups (and
 * at most one per CU), so that a few tiles per workgroup are reached with few queries.  Closed-form tables only; both
 * pointers 16-byte aligned; phases 1, 2, 4 or 8; max_workgroups >= 1; else MI_ERR_INVALID_ARG.  Counted by
 * mi_debug_sweep_ds_launches. */
mi_status mi_debug_interp1_phased_sweep(mi_ctx* ctx, const mi_grid1* g, const double* xq_dev, double* yq_dev,
                                        size_t nq, double extrap_val, int phases, int max_workgroups);
/* The same hook with the form of the phase shift chosen by the caller.  mi_debug_interp1_phased_sweep always runs the
 * clock form (class c waits c/phases of a tile period before its first load, whole tiles of 16384 queries).
 * first_units != 0 runs the shift by work instead: a decimal digit 1..4 per class, class 0 first (4123 = {4, 1, 2, 3}),
 * the number of 4096-query units in the first tile of a workgroup of that class; phases must be 1, 2 or 4 then and
 * nobody waits.  first_units == 0 is the clock form.  stamps_dev: NULL, or device memory for max_workgroups * stamp_cap
 * values (stamp_cap >= 2): workgroup b writes the wall clock to stamps_dev[b * stamp_cap + slot] at entry (slot 0), at
 * the start of the gather step of its tile i (slot 1 + i) and at exit (slot 1 + its tile count); slots beyond stamp_cap
 * are dropped, slots nobody writes keep their contents.  Results are the same bytes in every form. */
mi_status mi_debug_interp1_phased_sweep_ex(mi_ctx* ctx, const mi_grid1* g, const double* xq_dev, double* yq_dev,
                                           size_t nq, double extrap_val, int phases, int max_workgroups,
                                           unsigned first_units, unsigned long long* stamps_dev, unsigned stamp_cap);
/* Which queries the workgroup of a rank owns under the shift by work (csrc/mi_sweep_partition.hpp, the function the
 * kernel itself calls; no device is touched).  All starts are in units of 4096 queries.  Tile i of the workgroup starts
 * at  i == 0 ? first_start : i == ntiles-1 ? last_start : i == ntiles-2 ? pen_start : mid_origin + (i-1) mid_step  and
 * has  i == 0 ? first_tile_units : i == ntiles-1 ? last_tile_units : 4  units; work is the sum.  The nq % 4096 queries
 * behind the last unit belong to rank nwg - 1.  Any out pointer may be NULL.  MI_ERR_INVALID_ARG unless phases is 1, 2
 * or 4, first_units has that many digits 1..4 and rank < nwg. */
mi_status mi_debug_sweep_partition(size_t nq, unsigned nwg, int phases, unsigned first_units, unsigned rank,
                                   unsigned* ntiles, unsigned* first_tile_units, unsigned* last_tile_units, size_t* work,
                                   size_t* first_start, size_t* mid_origin, size_t* mid_step, size_t* pen_start,
                                   size_t* last_start);
/* Host convenience used by the arma::vec wrapper: uploads xq, runs, downloads
 * (synchronous). */
mi_status mi_interp1_f64_host(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq,
                              size_t nq, double extrap_val);
/* One-shot arma::interp1(X,Y,XI,YI,"linear",extrap) equivalent on host
 * pointers (sanitises X, builds a temporary table, synchronous). */
mi_status mi_interp1_f64(mi_ctx* ctx, const double* x, const double* y, size_t n, const double* xq,
                         double* yq, size_t nq, double extrap_val);

/* ---- 1-D interpolation, arma::interp1's "nearest" method ------------------
 * yq[i] = Y[k], k the node the nearest rule at the top of this header picks for xq[i].  The calls take the SAME
 * mi_grid1 handles as the linear calls: table construction, the four table modes, the closed forms and
 * MI_GRID_SANITISE are untouched, and one table serves both methods.  A table of labels or states, a zero-order-hold
 * resampling, a table with a NaN node (a linear lookup turns both neighbouring cells into NaN; nearest returns NaN only
 * for the queries closest to that node).
 * Each call copies the contract of the linear call it mirrors -- mi_interp1_f64_dev, mi_interp1_f64_host,
 * mi_interp1_f64 (which sanitises X; "nearest"), in that order: argument checks and status codes, 8-B alignment,
 * nq == 0 is MI_OK with nothing launched, 64-bit indexing, the device form asynchronous on the context's stream without
 * allocation, copy or synchronisation (capturable).  Algorithmic HBM bytes per query: 8 (xq) + 8 (yq); a closed-form
 * table (mode 0) is read with ONE 8-B gather per query, half the linear blend's table traffic.
 * Kernel choice (csrc/mi_nearest1.hip; mi_debug_nearest_launches tells which) is by alignment, table size and
 * mi_ctx_set_query_order only: MI_QUERIES_ORDERED -> the streaming kernel; MI_QUERIES_RANDOM or MI_QUERIES_AUTO -> the
 * whole-table-in-LDS kernel where the linear dispatcher's window admits it (table <= 128 KiB, nq >= 2^20), else the
 * streaming kernel; pointers that are not 16-B aligned -> the scalar kernel.  The nearest calls never read or write the
 * context's order probe, so they never change which kernel a later linear call launches.
 * Which call when: nearest-node lookup -> these calls.  There is NO region-sweep form of nearest: unordered queries over
 * a table larger than L2 take the streaming kernel here, and may then be SLOWER than mi_interp1_f64_dev, whose region
 * sweep orders such queries by table region; ordered or clustered queries, and tables that fit L2, stream as the linear
 * call does.  Many tables at once: one X, a table per column -> mi_interp1_cols_nearest_f64_dev; one X, a table per ROW
 * or the slices of a cube -> mi_interp1_rows_nearest_f64_dev; an X per column -> mi_interp1_pairs_nearest_f64_dev.
 * There is no nearest form of the each and rowpairs calls. */
mi_status mi_interp1_nearest_f64_dev(mi_ctx* ctx, const mi_grid1* g, const double* xq_dev, double* yq_dev,
                                     size_t nq, double extrap_val);
/* host pointers, synchronous: the chunked, pinned path of mi_interp1_f64_host around the nearest kernels */
mi_status mi_interp1_nearest_f64_host(mi_ctx* ctx, const mi_grid1* g, const double* xq, double* yq,
                                      size_t nq, double extrap_val);
/* One-shot arma::interp1(X,Y,XI,YI,"nearest",extrap) equivalent on host pointers (sanitises X, builds a temporary
 * table, synchronous). */
mi_status mi_interp1_nearest_f64(mi_ctx* ctx, const double* x, const double* y, size_t n, const double* xq,
                                 double* yq, size_t nq, double extrap_val);

/* ---- 2-D tables and scattered bilinear interpolation ------------------
 * z is column-major ny x nx, i.e. arma::mat(ny, nx).memptr(): z[i + j*ny] =
 * Z(y_i, x_j).  Blend along y inside the two bracketing columns, then along
 * x (oracle/interp_oracle.c orc_interp2_bilinear).  No counterpart in the
 * reference (BASELINE.json config 3). */
/* flags: MI_GRID_DEVICE_PTRS (z, x, y are device pointers); MI_GRID2_COMPACT keeps the resident table at 2x the
 * input bytes (column pairs) instead of the default 4x (quad cells: one 64-B sector per query, ~8 % faster). */
#define MI_GRID2_COMPACT 0x4u
mi_status mi_grid2_create(mi_ctx* ctx, const double* x, size_t nx, const double* y, size_t ny,
                          const double* z, unsigned flags, mi_grid2** out);
mi_status mi_grid2_create_uniform(mi_ctx* ctx, double x0, double dx, size_t nx, double y0, double dy,
                                  size_t ny, const double* z, unsigned flags, mi_grid2** out);
mi_status mi_grid2_destroy(mi_grid2* g);
/* resident bytes of the table */
mi_status mi_grid2_info(const mi_grid2* g, size_t* table_bytes);
mi_status mi_interp2_f64_dev(mi_ctx* ctx, const mi_grid2* g, const double* xq_dev,
                             const double* yq_dev, double* zq_dev, size_t nq, double extrap_val);
mi_status mi_interp2_f64_host(mi_ctx* ctx, const mi_grid2* g, const double* xq, const double* yq,
                              double* zq, size_t nq, double extrap_val);
/* Gridded form, arma::interp2(X, Y, Z, XI, YI, ZI): zi is column-major nyi x nxi, i.e.
 * arma::mat(nyi, nxi).memptr(), zi[i + j*nyi] = Z at (xi[j], yi[i]), bit-identical to mi_interp2_f64_dev on that
 * pair.  xi, yi need not be sorted.  Each coordinate is located once per call (records in a workspace the context
 * owns, grown on demand); the output is written once.  _dev: device pointers, 8-B aligned, asynchronous on the
 * context's stream; nxi == 0 or nyi == 0 is MI_OK with nothing launched.  _host: host pointers, synchronous. */
mi_status mi_interp2_grid_f64_dev(mi_ctx* ctx, const mi_grid2* g, const double* xi_dev, size_t nxi,
                                  const double* yi_dev, size_t nyi, double* zi_dev, double extrap_val);
mi_status mi_interp2_grid_f64_host(mi_ctx* ctx, const mi_grid2* g, const double* xi, size_t nxi,
                                   const double* yi, size_t nyi, double* zi, double extrap_val);
/* Which call when: pairs in no pattern -> mi_interp2_f64_dev; every combination of two query axes -> the gridded call
 * (each coordinate located once).  The value of the nearest node in place of the blend (label maps, masks, material
 * indices, a field with a NaN cell that must not spread) -> the nearest twins below. */

/* ---- arma::interp2's "nearest" method on a mi_grid2 -----------------------
 * The 2-D nearest rule at the top of this header in place of the blend: zq[i] = Z(ky, kx), a copy of one table element,
 * read from the resident (repacked) table of the linear calls -- the same handles, either layout, no second copy of Z.
 * Each call takes its linear twin's signature and its contract word for word: argument checks and status codes, 8-B
 * alignment, empty calls (nq == 0; nxi == 0 or nyi == 0) MI_OK with nothing launched or written, the overflow checks,
 * _dev asynchronous on the context's stream, _host synchronous.  xi, yi, xq, yq may be in any order.
 *   mi_interp2_nearest_f64_dev        scattered pairs (mi_interp2_f64_dev): one 8-B gather per query.
 *   mi_interp2_grid_nearest_f64_dev   gridded (mi_interp2_grid_f64_dev), zi column-major nyi x nxi,
 *                                     zi[i + j*nyi] == what mi_interp2_nearest_f64_dev returns for (xi[j], yi[i]), bit for
 *                                     bit.  Each coordinate becomes one 4-B record (node, or a flag) in the context's
 *                                     record workspace, shared in stream order with the linear calls: linear and nearest
 *                                     calls back to back do not disturb each other.  One 8-B read per output where the
 *                                     bilinear call reads 32 B, and none while the table column stays the same.
 *   mi_interp2_grid_nearest_f64_host  host pointers, synchronous: upload, the device call, download; beyond 2 x 8 Mi
 *                                     outputs in column chunks of about 8 Mi outputs on the context's own stream (no
 *                                     pinning, no second stream: the path is PCIe-bound either way).
 * Kernels: csrc/mi_nearest2.hip; mi_debug_nearest2_launches tells which body ran.  Timings against the linear twins:
 * not measured yet.  There are no group forms and no host form of the scattered call. */
mi_status mi_interp2_nearest_f64_dev(mi_ctx* ctx, const mi_grid2* g, const double* xq_dev,
                                     const double* yq_dev, double* zq_dev, size_t nq, double extrap_val);
mi_status mi_interp2_grid_nearest_f64_dev(mi_ctx* ctx, const mi_grid2* g, const double* xi_dev, size_t nxi,
                                          const double* yi_dev, size_t nyi, double* zi_dev, double extrap_val);
mi_status mi_interp2_grid_nearest_f64_host(mi_ctx* ctx, const mi_grid2* g, const double* xi, size_t nxi,
                                           const double* yi, size_t nyi, double* zi, double extrap_val);

/* ---- interp1 over the columns of a matrix (one X, many Y) ---------------
 * MATLAB's interp1 with a matrix Y; arma::interp1 takes vectors only, so this is the loop over the columns of an
 * arma::mat that its callers write.  y is column-major n x ncols with leading dimension ldy >= n
 * (arma::mat(n, ncols).memptr(), ldy = n), xi holds nxi queries in any order, yi is column-major nxi x ncols with
 * leading dimension ldyi >= nxi:
 *     yi[i + c*ldyi] == what mi_interp1_f64_dev returns for xi[i] on the table (x, y[:, c]),  bit for bit
 * (extrap_val outside [x[0], x[n-1]], NaN for a NaN query, y[n-1, c] at x[n-1]; inf / NaN / -0.0 inside a column go
 * through the two-term blend above and never reach another column).  Rows n..ldy-1 of y are never read, rows
 * nxi..ldyi-1 of yi are never written.
 *
 * The axis is a handle of its own -- validated and uploaded once, reused while y changes from call to call.  x is NOT
 * sorted or de-duplicated for the caller (that would mean permuting the rows of every y): this is Armadillo's
 * "*linear" contract, and a non-increasing or non-finite x is MI_ERR_GRID, as mi_grid1_create without
 * MI_GRID_SANITISE.  mi_axis1_create: flags = 0 or MI_GRID_DEVICE_PTRS (x is a device pointer, copied to the host
 * once for validation).  mi_axis1_create_uniform: nodes fma(i, dx, x0), as mi_grid1_create_uniform.
 *
 * _dev: device pointers, 8-B aligned, asynchronous on the context's stream; allocates only to grow the context's
 * record workspace (16 B per query, shared with mi_interp2_grid_f64_dev in stream order); ncols == 0 or nxi == 0 is
 * MI_OK with nothing launched.  _host: host pointers, synchronous, columns go through in chunks.
 * Which call when: many columns over one axis -> this call (each column is read once, each output written once).
 * A single column with many queries (ncols == 1) is served faster by a mi_grid1 and mi_interp1_f64_dev, whose
 * kernels read the queries and the table directly instead of going through 16-B records. */
mi_status mi_axis1_create(mi_ctx* ctx, const double* x, size_t n, unsigned flags, mi_axis1** out);
mi_status mi_axis1_create_uniform(mi_ctx* ctx, double x0, double dx, size_t n, mi_axis1** out);
mi_status mi_axis1_destroy(mi_axis1* axis);
mi_status mi_interp1_cols_f64_dev(mi_ctx* ctx, const mi_axis1* axis, const double* y_dev, size_t ldy, size_t ncols,
                                  const double* xi_dev, size_t nxi, double* yi_dev, size_t ldyi, double extrap_val);
mi_status mi_interp1_cols_f64_host(mi_ctx* ctx, const mi_axis1* axis, const double* y, size_t ldy, size_t ncols,
                                   const double* xi, size_t nxi, double* yi, size_t ldyi, double extrap_val);
/* The "nearest" method over the columns of a matrix: mi_interp1_cols_f64_dev's contract word for word (layouts, argument
 * checks and status codes, 8-B alignment, ncols == 0 or nxi == 0 is MI_OK with nothing launched, rows n..ldy-1 of y never
 * read, rows nxi..ldyi-1 of yi never written, asynchronous on the context's stream) with the nearest rule in place of the
 * blend:
 *     yi[i + c*ldyi] == what mi_interp1_nearest_f64_dev returns for xi[i] on the table (x, y[:, c]),  bit for bit
 * -- the stored value of the nearest node, inf / NaN / -0.0 as they are.  Each query is located once per call into one
 * int32 (4 B per query in the context's record workspace -- the slot the linear call's 16-B records use, in stream order,
 * grown on demand: linear and nearest calls back to back do not disturb each other); one kernel follows, which stages each
 * column once in LDS for n <= 8192 and gathers y[k, c] through L2 for longer columns (mi_debug_nearest_launches: 3 / 4).
 * There is no host-pointer, group or arma:: form of this call: like the host forms of the row calls they wait for the
 * cause of the open fault on the strided host-copy path. */
mi_status mi_interp1_cols_nearest_f64_dev(mi_ctx* ctx, const mi_axis1* axis, const double* y_dev, size_t ldy, size_t ncols,
                                          const double* xi_dev, size_t nxi, double* yi_dev, size_t ldyi, double extrap_val);

/* ---- interp1 over paired columns (an X per column of Y) -------------------
 * A batch of independent tables that all answer the same queries: column c of y is sampled at the nodes in column c of
 * x.  An ensemble of trajectories, each recorded at its own (event) times, resampled onto one common mesh; with n = 2
 * and nxi = 1 it is the shape of the reference's RestrictKernel (EventDrivenMap.cu:769-785) in fp64.  x (leading
 * dimension ldx >= n), y (ldy >= n) and yi (ldyi >= nxi) are column-major; len (optional, NULL: n everywhere) holds one
 * uint32 per column, the number n_c of valid leading rows of that column, 2 <= n_c <= n:
 *     yi[i + c*ldyi] == what mi_interp1_f64_dev returns for xi[i] on the table (x[0:n_c, c], y[0:n_c, c]) built
 *                       without MI_GRID_SANITISE,  bit for bit
 * (the fp64 blend above; extrap_val outside [x[0, c], x[n_c-1, c]], NaN for a NaN query; inf / NaN / -0.0 inside a
 * column of y go through the two-term blend and never reach another column).  Rows n_c..ldx-1 of x and n_c..ldy-1 of y
 * never influence anything, rows nxi..ldyi-1 of yi are never written.
 *
 * x changes from call to call and lives on the device, so it is validated on the device, at every call, with
 * mi_axis1_create's rule.  A column is BAD when n_c < 2, n_c > n, any of x[0:n_c, c] is not finite, or x[0:n_c, c] is not
 * strictly increasing (!(x[k-1] < x[k]): equal nodes and the pair -0.0, 0.0 are bad; x is never sorted for the caller).
 * All nxi outputs of a bad column are NaN whatever the queries and extrap_val; no other column is affected.  col_ok
 * (optional) receives one uint32 per column: 1 good, 0 bad.
 *
 * _dev: device pointers; doubles 8-B aligned, len / col_ok 4-B aligned; 2 <= n < 2^31 - 16; asynchronous on the
 * context's stream, no copy, no synchronisation; ncols == 0 or nxi == 0 is MI_OK with nothing launched or written.
 * MI_ERR_INVALID_ARG for NULL or misaligned pointers, ldx < n, ldy < n, ldyi < nxi, n < 2, sizes whose byte counts
 * overflow.  Allocation: none for n <= 4096 (columns are staged and validated in LDS).  For longer columns a validation
 * pass writes one flag per column first: into col_ok_dev when the caller gave one, otherwise into the context's record
 * workspace (4 B per column, grown on demand, shared in stream order with mi_interp2_grid_f64_dev and
 * mi_interp1_cols_f64_dev) -- so with col_ok_dev the call never allocates.
 * _host: host pointers, synchronous, columns go through in pinned, pipelined chunks.  Every output is complete either
 * way; the status is MI_ERR_GRID (the text names the first bad column) when at least one column is bad and col_ok is
 * NULL, MI_OK when col_ok was given.
 * Which call when: one X for every column -> mi_interp1_cols_f64_dev (it locates each query once per call); an X per
 * column -> this call; one column with many queries -> mi_grid1 and mi_interp1_f64_dev; the same data stored the other
 * way round, an X per ROW -> mi_interp1_rowpairs_f64_dev, without a transpose; the node closest to each query in
 * place of the blend (labels, states, values that must not be averaged) -> mi_interp1_pairs_nearest_f64_dev, also for
 * very short columns: it has no thin form, and the Restrict shape n = 2 goes through its LDS form. */
mi_status mi_interp1_pairs_f64_dev(mi_ctx* ctx, const double* x_dev, size_t ldx, const double* y_dev, size_t ldy, size_t n,
                                   const uint32_t* len_dev, size_t ncols, const double* xi_dev, size_t nxi,
                                   double* yi_dev, size_t ldyi, double extrap_val, uint32_t* col_ok_dev);
mi_status mi_interp1_pairs_f64_host(mi_ctx* ctx, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                    const uint32_t* len, size_t ncols, const double* xi, size_t nxi, double* yi,
                                    size_t ldyi, double extrap_val, uint32_t* col_ok);
/* The "nearest" method over paired columns: mi_interp1_pairs_f64_dev's contract word for word (layouts, len and n_c, the
 * BAD-column rule -- all nxi outputs of a bad column are NaN -- col_ok, argument checks and status codes with this
 * function's name in the text, alignment, ncols == 0 or nxi == 0 is MI_OK with nothing launched or written, rows behind
 * n_c never reach a result, asynchronous on the context's stream) with the nearest rule in place of the blend:
 *     yi[i + c*ldyi] == what mi_interp1_nearest_f64_dev returns for xi[i] on the table (x[0:n_c, c], y[0:n_c, c]) built
 *                       without MI_GRID_SANITISE,  bit for bit
 * -- the stored value of the nearest node, inf / NaN / -0.0 as they are; a tie keeps the left node.  The state at the
 * event closest to each mesh time: labels, spike indices stored as doubles, any column whose values must not be averaged.
 * Allocation: none for n <= 4096 (columns are staged and validated in LDS; after the bracket search an output costs two
 * subtractions, a compare and one LDS read); for longer columns the validation flags go into col_ok_dev when given, else
 * into the context's record workspace (4 B per column), and y[k, c] is gathered once through L2
 * (csrc/mi_nearest_batched.hip; mi_debug_nearest_batched_launches: 3 / 4).  There is no thin form for very short columns:
 * n = 2 goes through the LDS form.  There is no host-pointer, group or arma:: form of this call. */
mi_status mi_interp1_pairs_nearest_f64_dev(mi_ctx* ctx, const double* x_dev, size_t ldx, const double* y_dev, size_t ldy,
                                           size_t n, const uint32_t* len_dev, size_t ncols, const double* xi_dev,
                                           size_t nxi, double* yi_dev, size_t ldyi, double extrap_val,
                                           uint32_t* col_ok_dev);

/* ---- interp1 over paired columns, a query vector per column ---------------
 * mi_interp1_pairs_f64_dev with an XI per column: an ensemble of independent tables, each with its own X, Y and XI.
 * Inverse-CDF sampling from ncols distributions (column c of x a CDF, of y its quantiles, of xi that distribution's
 * uniform draws); every trajectory resampled onto a time mesh of its own; Restrict with a horizon per realisation.
 * The contract is mi_interp1_pairs_f64_dev's word for word -- x, y, yi, len, n_c, the BAD-column rule (all nxi outputs
 * NaN, no other column affected), col_ok, alignment, the empty calls, the status rule of the _host form -- with one
 * change: xi is column-major nxi x ncols with leading dimension ldxi >= nxi, 8-B aligned, and
 *     yi[i + c*ldyi] == what mi_interp1_f64_dev returns for xi[i + c*ldxi] on the table (x[0:n_c, c], y[0:n_c, c]) built
 *                       without MI_GRID_SANITISE,  bit for bit.
 * Rows nxi..ldxi-1 of xi are never read; yi must not overlap an input.
 * ldxi == 0 means ONE xi vector (nxi doubles) for every column: the results are bit-identical to
 * mi_interp1_pairs_f64_dev's.  0 < ldxi < nxi is MI_ERR_INVALID_ARG, and ldxi takes part in the byte-count overflow check.
 * Very short columns (n and nxi both small; the reference's RestrictKernel shape n = 2, nxi = 1 among them) are served
 * by a thin kernel, one lane per column, whatever ldxi is -- for one shared xi this call with ldxi == 0 is the way to it;
 * longer columns with ldxi == 0 are handed to mi_interp1_pairs_f64_dev unchanged.
 * _dev: asynchronous on the context's stream, no copy, no synchronisation.  Allocation: none for n <= 4096; for longer
 * columns with ldxi > 0 the validation flags go into col_ok_dev when given, otherwise into the context's record
 * workspace, exactly as in mi_interp1_pairs_f64_dev.
 * _host: host pointers, synchronous, pinned and pipelined column chunks; with ldxi > 0 xi travels with its columns.
 * Which call when: an X AND an XI per column, or very short columns (n <= 32 and nxi <= 8: kThinMaxN, kThinMaxQ in csrc/mi_each1.hip) -> this call; an X per column
 * and one XI -> mi_interp1_pairs_f64_dev; one X for every column -> mi_interp1_cols_f64_dev. */
mi_status mi_interp1_each_f64_dev(mi_ctx* ctx, const double* x_dev, size_t ldx, const double* y_dev, size_t ldy, size_t n,
                                  const uint32_t* len_dev, size_t ncols, const double* xi_dev, size_t ldxi, size_t nxi,
                                  double* yi_dev, size_t ldyi, double extrap_val, uint32_t* col_ok_dev);
mi_status mi_interp1_each_f64_host(mi_ctx* ctx, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                   const uint32_t* len, size_t ncols, const double* xi, size_t ldxi, size_t nxi, double* yi,
                                   size_t ldyi, double extrap_val, uint32_t* col_ok);

/* ---- gridded interp2 over the slices of a cube, Z read in place -------------
 * arma::interp2 in a loop over the slices of an arma::cube: an ensemble of 2-D fields regridded onto another mesh, a
 * field that lives on the device and changes from step to step.  Two axes (mi_axis1: nx = ax->n and ny = ay->n nodes;
 * ax == ay is allowed) and a stack of nslices plain column-major matrices, the layout of
 * arma::cube(ny, nx, nslices).memptr():
 *     Z_s(i, j) = z[i + j*ldz + s*z_slice_stride],     ny x nx,   ldz >= ny,   z_slice_stride >= ldz*nx,
 *     ZI_s(i, j) = zi[i + j*ldzi + s*zi_slice_stride], nyi x nxi, ldzi >= nyi, zi_slice_stride >= ldzi*nxi
 * (both strides are ignored for nslices <= 1), and
 *     zi[i + j*ldzi + s*zi_slice_stride] == what mi_interp2_grid_f64_dev returns at (xi[j], yi[i]) on a mi_grid2 built
 *                                           from (x, y, Z_s),  bit for bit:
 * oracle/interp_oracle.c orc_interp2_bilinear -- the four corners Z(ly,lx), Z(ry,lx), Z(ly,rx), Z(ry,rx) with
 * r = min(l+1, n-1), the blend along y inside both columns, then along x, every product and sum rounded (no FMA),
 * extrap_val outside either axis, NaN for a NaN coordinate.  xi and yi may be in any order.  Rows ny..ldz-1 of z and the
 * gap between slices are never read; rows nyi..ldzi-1 of zi and the gap between slices are never written; zi must not
 * overlap an input.  inf, NaN and -0.0 inside a slice go through the blend; they never reach another slice, or an output
 * whose four corners do not include them.
 * _dev: device pointers, 8-B aligned; asynchronous on the context's stream, no copy, no synchronisation; the only
 * allocation grows the context's record workspace ((nxi + nyi) x 16 B, shared in stream order with
 * mi_interp2_grid_f64_dev, mi_interp1_cols_f64_dev and the long-column forms of the paired-column calls); nslices == 0,
 * nxi == 0 or nyi == 0 is MI_OK with nothing launched or written.  Each coordinate is located once per call for all
 * slices; one kernel follows, which reads each slice once into LDS when it holds at most 8192 elements and gathers the
 * corners from the slice itself otherwise (csrc/mi_slices2.hip; mi_debug_slices2_launches tells which).
 * MI_ERR_INVALID_ARG for NULL or misaligned pointers, an axis of another device than the context's, ldz < ny,
 * ldzi < nyi, a slice stride smaller than its matrix (nslices > 1), sizes whose byte counts overflow.
 * There is no host-pointer or group form of this call yet.
 * Which call when: one table that answers many calls -> mi_grid2 and mi_interp2_grid_f64_dev (its resident layout gives
 * one 32-B cell per output); a Z that changes on the device, or many slices over one pair of axes -> this call.  The
 * value of the nearest node in place of the blend -> mi_interp2_slices_nearest_f64_dev. */
mi_status mi_interp2_slices_f64_dev(mi_ctx* ctx, const mi_axis1* ax, const mi_axis1* ay, const double* z_dev, size_t ldz,
                                    size_t z_slice_stride, size_t nslices, const double* xi_dev, size_t nxi,
                                    const double* yi_dev, size_t nyi, double* zi_dev, size_t ldzi, size_t zi_slice_stride,
                                    double extrap_val);
/* The "nearest" method over the slices of a cube: mi_interp2_slices_f64_dev's contract word for word (layouts, argument
 * checks and status codes, 8-B alignment, the axis-device check, the overflow checks, both strides ignored for
 * nslices <= 1, empty calls MI_OK with nothing launched or written, rows ny..ldz-1 of z and the gap between slices never
 * read, rows nyi..ldzi-1 of zi and the gap between slices never written, asynchronous on the context's stream) with the
 * 2-D nearest rule in place of the blend:
 *     zi[i + j*ldzi + s*zi_slice_stride] == z[ky + kx*ldz + s*z_slice_stride],  the stored 64 bits,
 * bit-identical to mi_interp2_grid_nearest_f64_dev on a mi_grid2 built from (x, y, Z_s).  A special value in one slice
 * reaches the outputs of that slice whose (ky, kx) is its node and nothing else.  Each coordinate is located once per call
 * for all slices (4-B records in the context's record workspace, shared in stream order with the linear calls); one
 * kernel follows, which gathers through L2 for every slice size: one 8-B read per output where the linear call reads
 * four corners, so there is no LDS form (csrc/mi_nearest2.hip; mi_debug_nearest2_launches: 5 / 6 / 7).  Timing against
 * the linear LDS form for small slices: not measured yet. */
mi_status mi_interp2_slices_nearest_f64_dev(mi_ctx* ctx, const mi_axis1* ax, const mi_axis1* ay, const double* z_dev, size_t ldz,
                                            size_t z_slice_stride, size_t nslices, const double* xi_dev, size_t nxi,
                                            const double* yi_dev, size_t nyi, double* zi_dev, size_t ldzi,
                                            size_t zi_slice_stride, double extrap_val);

/* ---- interp1 along the rows of a matrix / across the slices of a cube -------
 * mi_interp1_cols_f64_dev for data stored the other way round: one table per ROW of a column-major matrix.  An ensemble
 * stored realisation-fastest, one time level per contiguous block (the reference's [spike][realisation] arrays, index
 * m*R + r); a stack of fields at n time levels, arma::cube(ny, nx, n).memptr(), interpolated to other times (m = ny*nx
 * rows, ldy = the slice stride); a C-contiguous (n, B) "time-major" tensor.
 *     y:  column-major m x n,   n = axis->n,  Y(r, k) = y[r + k*ldy],  ldy >= m,
 *     yi: column-major m x nxi,               yi[r + i*ldyi],          ldyi >= m,
 *     yi[r + i*ldyi] == what mi_interp1_f64_dev returns for xi[i] on the table (x, Y(r, :)) built without
 *                       MI_GRID_SANITISE,  bit for bit:
 * the fp64 blend at the top of this header, (1-w)*Y(r,l) + w*Y(r,rr) with rr = min(l+1, n-1), every operation rounded;
 * extrap_val outside [x[0], x[n-1]]; NaN for a NaN query; Y(r, n-1) goes through the blend at x[n-1]; inf, NaN and -0.0
 * inside a row go through the blend and never reach another row.  xi may be in any order.  Rows m..ldy-1 of every column
 * of y never influence anything, rows m..ldyi-1 of yi are never written; yi must not overlap an input.
 * Device form only: device pointers, 8-B aligned; asynchronous on the context's stream, no copy, no synchronisation; the
 * only allocation grows the context's record workspace (nxi x 16 B, shared in stream order with mi_interp2_grid_f64_dev,
 * mi_interp1_cols_f64_dev, mi_interp2_slices_f64_dev and the long-column forms of the paired-column calls); m == 0 or
 * nxi == 0 is MI_OK with nothing launched or written.  Each query is located once per call; one kernel follows, in which
 * a workgroup keeps the two bracketing columns of its 1024 rows in registers, so that with sorted xi every column of y a
 * query brackets is read once and the others never; for m < 256 a flat kernel takes the record per output
 * (csrc/mi_rows1.hip; mi_debug_rows1_launches tells which).  With xi in no order two columns are read per output.
 * MI_ERR_INVALID_ARG for NULL or misaligned pointers, an axis of another device than the context's, ldy < m, ldyi < m,
 * sizes whose byte counts overflow (ldy*n, ldyi*nxi, nxi*16).
 * There is no host-pointer, group or arma:: form of this call.
 * Which call when: one table per ROW, or interpolation across the slices of a cube -> this call; one table per column ->
 * mi_interp1_cols_f64_dev; a single row with many queries (m == 1) -> mi_grid1 and mi_interp1_f64_dev; one table per row
 * AND an X per row -> mi_interp1_rowpairs_f64_dev; the snapshot closest in time (a zero-order hold across the slices of
 * a cube) in place of the blend -> mi_interp1_rows_nearest_f64_dev. */
mi_status mi_interp1_rows_f64_dev(mi_ctx* ctx, const mi_axis1* axis, const double* y_dev, size_t ldy, size_t m,
                                  const double* xi_dev, size_t nxi, double* yi_dev, size_t ldyi, double extrap_val);
/* The "nearest" method along the rows of a matrix / across the slices of a cube: mi_interp1_rows_f64_dev's contract word
 * for word (layouts, argument checks and status codes with this function's name in the text, 8-B alignment, m == 0 or
 * nxi == 0 is MI_OK with nothing launched or written, rows m..ldy-1 of y never read, rows m..ldyi-1 of yi never written,
 * the axis-device check, asynchronous on the context's stream) with the nearest rule in place of the blend:
 *     yi[r + i*ldyi] == what mi_interp1_nearest_f64_dev returns for xi[i] on the table (x, Y(r, :)),  bit for bit
 * -- the stored value of the nearest node, inf / NaN / -0.0 as they are, and bit-identical to
 * mi_interp1_cols_nearest_f64_dev on the transposed data.  A NaN or inf snapshot reaches the queries of its own two
 * half-cells only, where the linear call loses both neighbouring cells.  Each query is located once per call into one
 * int32 (nxi x 4 B in the context's record workspace, the slot of the linear calls' records, in stream order with them:
 * linear and nearest calls back to back do not disturb each other); one kernel follows, in which an output column is a
 * copy of ONE input column: a workgroup keeps one column of its 1024 rows in registers, so that with sorted xi every
 * column of y some query is nearest to is read once and the others never, and with xi in no order ONE column is read per
 * output (the linear call: two); for m < 256 a flat kernel gathers one value per output (csrc/mi_nearest_batched.hip;
 * mi_debug_nearest_batched_launches: 0 / 1 / 2).  Algorithmic bytes: 8*m*(columns touched) + 8*m*nxi + 8*nxi.
 * MI_ERR_INVALID_ARG also for sizes whose byte counts overflow (ldy*n, ldyi*nxi, nxi*4).
 * There is no host-pointer, group or arma:: form of this call. */
mi_status mi_interp1_rows_nearest_f64_dev(mi_ctx* ctx, const mi_axis1* axis, const double* y_dev, size_t ldy, size_t m,
                                          const double* xi_dev, size_t nxi, double* yi_dev, size_t ldyi,
                                          double extrap_val);

/* ---- interp1 over paired rows (an X per row of Y) ---------------------------
 * mi_interp1_pairs_f64_dev for data stored the other way round: row r of y is sampled at the nodes in row r of x.  An
 * ensemble stored realisation-fastest, one time level per contiguous block (the reference's [spike][realisation] event
 * arrays, index m*R + r), every trajectory recorded at its own event times, resampled onto one common mesh where it
 * lies; with n = 2 and nxi = 1 it is the shape of the reference's RestrictKernel in fp64.  The contract is
 * mi_interp1_pairs_f64_dev's word for word, with rows in place of columns:
 *     x:  column-major m x n,    X(r, k) = x[r + k*ldx],  ldx >= m,
 *     y:  column-major m x n,    Y(r, k) = y[r + k*ldy],  ldy >= m,
 *     yi: column-major m x nxi,  yi[r + i*ldyi],          ldyi >= m,
 * len (optional, NULL: n everywhere) holds one uint32 per row, the number n_r of valid leading nodes of that row,
 * 2 <= n_r <= n; xi holds nxi queries in any order, shared by every row:
 *     yi[r + i*ldyi] == what mi_interp1_f64_dev returns for xi[i] on the table (X(r, 0:n_r), Y(r, 0:n_r)) built without
 *                       MI_GRID_SANITISE,  bit for bit
 * (the fp64 blend at the top of this header, (1-w)*Y(r,l) + w*Y(r,rr) with rr = min(l+1, n_r-1), every operation rounded,
 * no FMA; extrap_val outside [X(r,0), X(r,n_r-1)], NaN for a NaN query; inf / NaN / -0.0 inside a row of y go through the
 * two-term blend and never reach another row).  Nodes k >= n_r of a row, rows m..ld-1 of any operand and padding never
 * influence anything; rows m..ldyi-1 of yi are never written; yi must not overlap an input.
 *
 * x is validated on the device, at every call, with mi_axis1_create's rule.  A row is BAD when n_r < 2, n_r > n, any of
 * X(r, 0:n_r) is not finite, or X(r, 0:n_r) is not strictly increasing (!(X(r,k-1) < X(r,k)): equal nodes and the pair
 * -0.0, 0.0 are bad; x is never sorted for the caller).  All nxi outputs of a bad row are NaN whatever the queries and
 * extrap_val; no other row is affected.  row_ok (optional) receives one uint32 per row: 1 good, 0 bad.  Bad rows are
 * data, found asynchronously: the status is MI_OK.
 *
 * Device form only: device pointers; doubles 8-B aligned, len / row_ok 4-B aligned; 2 <= n < 2^31 - 16; asynchronous on
 * the context's stream, no copy, no synchronisation; m == 0 or nxi == 0 is MI_OK with nothing launched or written.
 * MI_ERR_INVALID_ARG for NULL or misaligned pointers, ldx < m, ldy < m, ldyi < m, n < 2, sizes whose byte counts overflow
 * (ldx*n, ldy*n, ldyi*nxi, m*4).  A lane owns a row and marches along it as the (shared) queries go by; sorted xi makes
 * that one pass over x and y, any other order stays correct and costs a binary search of the row per jump
 * (csrc/mi_rowpairs1.hip; mi_debug_rowpairs_launches tells the form).  Allocation: none for n <= 32 (rows are validated
 * inside the one kernel).  For longer rows a validation pass writes one flag per row first: into row_ok_dev when the
 * caller gave one, otherwise into the context's record workspace (4 B per row, grown on demand, shared in stream order
 * with mi_interp2_grid_f64_dev, mi_interp1_cols_f64_dev, mi_interp1_rows_f64_dev, mi_interp2_slices_f64_dev and the
 * long-column forms of the paired-column calls) -- so with row_ok_dev the call never allocates, and it can be captured
 * into a hipGraph once any workspace has grown.
 * Out of scope: there is no host-pointer, group or arma:: form of this call (they wait for the cause of the open fault on
 * the strided host-copy path; this call adds no host upload path), no query vector per row,
 * and no fp32 form.
 * Which call when: an X per ROW (realisation-fastest data), many rows, xi sorted or nearly so -> this call (measured
 * 1.3-2.8x the transposing route); an X per column -> mi_interp1_pairs_f64_dev; one X for all rows ->
 * mi_interp1_rows_f64_dev.  Two shapes are better served by a transpose and mi_interp1_pairs_f64_dev: xi in no order with
 * long rows (this call then searches its row per output; measured 4x slower than that route at n = 1024), and a handful
 * of very long rows (a lane per row leaves the machine empty; m = 8: 19x slower). */
mi_status mi_interp1_rowpairs_f64_dev(mi_ctx* ctx, const double* x_dev, size_t ldx, const double* y_dev, size_t ldy,
                                      size_t m, size_t n, const uint32_t* len_dev, const double* xi_dev, size_t nxi,
                                      double* yi_dev, size_t ldyi, double extrap_val, uint32_t* row_ok_dev);

/* ---- the reference's own interpolation ----------------------------------
 * Replaces RestrictKernel (EventDrivenMap.cu:769-785, launch :205-206):
 *   x_k = -L + 2L/ngrid * ind_k ;  out = x0 + (T-t0)*(x1-x0)/(t1-t0)   (fp32)
 * Arrays are [spike][realisation] (index m*R + r), n = S*R elements.  `out`
 * may alias t0 (the reference works in place).  Device pointers.
 * The indices are read unsigned over the whole uint16 range, in any order
 * (i1 < i0 and indices >= ngrid are plain arithmetic, not errors).  There is no
 * guard for t1 == t0, exactly like the reference: the element is +-inf, or NaN
 * where the numerator is 0 too; NaN / inf times propagate.
 */
mi_status mi_restrict_f32_dev(mi_ctx* ctx, const float* t0, const uint16_t* i0, const float* t1,
                              const uint16_t* i1, float final_time, float half_length,
                              uint32_t ngrid, float* out, size_t n);
/* Host convenience (what the arma::fvec wrapper calls): uploads the four event arrays, runs, downloads
 * (synchronous).  out may alias t0. */
mi_status mi_restrict_f32_host(mi_ctx* ctx, const float* t0, const uint16_t* i0, const float* t1,
                               const uint16_t* i1, float final_time, float half_length, uint32_t ngrid,
                               float* out, size_t n);
/* Replaces CountRealisationsKernel + realisationReductionKernelBlocks
 * (EventDrivenMap.cu:787-824): mean over accepted realisations, per spike.
 * x: f32[nspikes*nreal] ([spike][realisation]), accept: u32[nreal] (0/1).
 * mean_dev: f32[nspikes]; count_dev: u32[1]; sums_dev (optional, may be
 * NULL): f64[MI_EDM_PARTIAL_LEN(nspikes)], the partial block
 *   [ sum_m over the accepted realisations, m < nspikes | accepted count | x0_m ]
 * whose element-wise sum over the shards of a multi-GPU run is what
 * mi_edm_residual_from_sums turns into the mean.
 * quirk != 0 reproduces the reference's accept[0] clobber
 * (EventDrivenMap.cu:800-802 overwrites accept[0] with the count, :817 then
 * tests accept[index]==1): realisation 0 is left out of the sums -- and
 * counted in the divisor (:822) -- unless count == 1, when it is summed whatever
 * its flag was.  In the partial block the sums never contain realisation 0 when
 * quirk is set and x0_m holds its restricted position (0 without quirk), so the
 * count == 1 rule can be applied to the total.  `accept` is never modified.
 * count = sum of the flags; only a flag equal to 1 puts its realisation into the
 * sums, so a flag > 1 is counted and not summed (that is what the clobbered
 * accept[0] is).  count == 0 gives count 0 and every mean NaN (0/0, what the
 * formula gives; with quirk too, realisation 0 re-enters for count == 1 only).
 * A rejected realisation is selected away, not multiplied by 0: its values may
 * be inf or NaN (Restrict with t1 == t0) without reaching a mean. */
#define MI_EDM_PARTIAL_LEN(nspikes) (2 * (nspikes) + 1)
mi_status mi_masked_mean_f32_dev(mi_ctx* ctx, const float* x, const uint32_t* accept, size_t nreal,
                                 size_t nspikes, int quirk, float* mean_dev, uint32_t* count_dev,
                                 double* sums_dev);
/* Fused Restrict + masked mean: one pass over the 4 event arrays, no
 * intermediate (what ComputeF uses).  restricted_dev may be NULL. */
mi_status mi_restrict_mean_f32_dev(mi_ctx* ctx, const float* t0, const uint16_t* i0, const float* t1,
                                   const uint16_t* i1, const uint32_t* accept, float final_time,
                                   float half_length, uint32_t ngrid, size_t nreal, size_t nspikes,
                                   int quirk, float* restricted_dev, float* mean_dev,
                                   uint32_t* count_dev, double* sums_dev);

/* ---- EventDrivenMap: the residual evaluation ------------------------------
 * Replaces class EventDrivenMap (EventDrivenMap.hpp:11-121,
 * EventDrivenMap.cu:57-404): lift -> evolve -> restrict -> average.
 */
typedef struct mi_edm_params {
    float vth, a1, a2, b1, b2, I, L;   /* parameters.hpp:1-8                     */
    double newton_tol;                 /* parameters.hpp:9  (tol, a double)      */
    uint32_t newton_max_iter;          /* counterMax: undefined in the reference
                                          (EventDrivenMap.cu:564); default 100   */
    uint32_t n_spikes;                 /* parameters.hpp:12 noSpikes (<= 8)      */
    float time_horizon;                /* parameters.hpp:15                      */
    uint32_t n_grid;                   /* mNoThreads (EventDrivenMap.cu:70), <= 1024 */
    uint32_t n_real;                   /* mNoReal                                */
    float beta_mean;                   /* (*pParameters)[0]                      */
    float beta_stddev;                 /* mParStdDev (EventDrivenMap.cu:105)     */
    uint64_t seed;                     /* mSeed                                  */
    int math_mode;                     /* MI_EDM_MATH_EXACT or MI_EDM_MATH_FAST  */
    int mean_quirk;                    /* default 1: average exactly as the
                                          reference does (EventDrivenMap.cu:800-802,
                                          :817,:822: realisation 0 is left out of the
                                          sum but counted in the divisor, unless only
                                          one realisation was accepted); 0: the true
                                          mean over the accepted realisations        */
    uint32_t max_events;               /* hard bound on events per realisation
                                          (termination guarantee; default 2^20)  */
    uint32_t real_offset;              /* global index of this shard's first
                                          realisation (multi-GPU sharding; only
                                          enters the per-neuron beta draw)       */
    uint32_t dedup_identical;          /* opt-in, default 0: with beta_stddev == 0
                                          every realisation is the same computation
                                          (the draw is the only per-realisation
                                          input, EventDrivenMap.cu:179,196); evolve
                                          one and replicate its events to all n_real
                                          rows.  Outputs are bit-identical to the
                                          full evolution; ignored when stddev != 0 */
} mi_edm_params;
#define MI_EDM_MATH_EXACT 0   /* software exp/log, bit-identical to oracle/edm_oracle.c */
#define MI_EDM_MATH_FAST  1   /* v_exp_f32 / v_log_f32 hardware transcendentals          */

void mi_edm_default_params(mi_edm_params* p);
mi_status mi_edm_create(mi_ctx* ctx, const mi_edm_params* p, mi_edm** out);
mi_status mi_edm_destroy(mi_edm* e);
/* setters of EventDrivenMap.hpp:27-51 arrive as a new parameter block */
mi_status mi_edm_set_params(mi_edm* e, const mi_edm_params* p);
/* Tuning / test knob; every choice gives bit-identical results (tests/test_edm_gpu.py runs each case under all of them).
 * waves_per_realisation: 0 = by realisation count (default: a workgroup of four waves per realisation for 48 up to
 * one realisation per CU, one wave per realisation otherwise), 1 or 4 = that form always.  uniform_division: 1 (default) = the
 * exact quotient in three or five operations (multiply by the divisor's rounded reciprocal + one or two correction steps;
 * one only where the device has proved it exact for that divisor) where a divisor is the same for the whole launch,
 * 0 = IEEE division everywhere. */
mi_status mi_edm_set_kernel_choice(mi_edm* e, int waves_per_realisation, int uniform_division);
/* ComputeF (EventDrivenMap.cu:154-240).  z: host, n_spikes doubles (c, Z1..);
 * f: host, n_spikes doubles.  partial (optional, may be NULL): host,
 * MI_EDM_PARTIAL_LEN(n_spikes) doubles receiving this device's partial block
 * [sums | accepted count | x0] (see mi_masked_mean_f32_dev) so that a caller
 * sharding realisations over GPUs can all-reduce them (the shard with
 * real_offset == 0 holds realisation 0 of the ensemble and is the only one that
 * applies mean_quirk); when partial is non-NULL f is still the single-device
 * residual. */
mi_status mi_edm_compute_f(mi_edm* e, const double* z, double* f, double* partial);
/* The same in two halves: _begin enqueues the whole evaluation on the context's stream and returns (with 600 or more
 * realisations it first waits for the lift kernel -- microseconds -- because the evolve kernel's LDS is sized by the
 * lift profile's live slices; the evolve kernel itself, which is > 99.9 % of the evaluation, is never waited for),
 * _end waits for it and forms f (and partial).  Independent evaluations -- the columns of NewtonSolver's
 * finite-difference Jacobian (NewtonSolver.cpp:178-197) -- can then overlap on the device: one mi_ctx (with its own
 * stream) and one mi_edm per evaluation in flight, _begin on all of them, _end on all of them.  One evaluation per
 * handle at a time. */
mi_status mi_edm_compute_f_begin(mi_edm* e, const double* z);
mi_status mi_edm_compute_f_end(mi_edm* e, double* f, double* partial);
/* f from the all-reduced (element-wise summed) partial blocks, MI_EDM_PARTIAL_LEN(n_spikes) doubles: the
 * averaging rule of p->mean_quirk applied to the totals, then the host arithmetic of EventDrivenMap.cu:237-239.
 * With one shard this reproduces mi_edm_compute_f's f bit for bit. */
mi_status mi_edm_residual_from_sums(const mi_edm_params* p, const double* z, const double* sums_and_count,
                                    double* f);
/* Debug taps (SaveLift/SaveEvolve/SaveRestrict, EventDrivenMap.cu:406-503):
 * copy stage outputs of the last compute_f to host.  Any pointer may be NULL.
 * v,s: f32[n_grid]; t0,t1,restricted: f32[S*R]; i0,i1: u16[S*R]; accept: u32[R] */
mi_status mi_edm_debug_read(mi_edm* e, float* v, float* s, float* w, float* t0, uint16_t* i0,
                            float* t1, uint16_t* i1, uint32_t* accept, float* restricted,
                            uint16_t* seed_ind);
/* Decision-coverage taps of the last compute_f (the device-side mirror of the oracle's orc_edm_counters,
 * oracle/edm_oracle.c): the evolve stage is run once more by an instantiation of the kernel that also counts
 *   [0] events of all realisations   [1] most events of one realisation   [2] most Newton iterations of one
 *   firing-time solve (eventTime, EventDrivenMap.cu:561-571)   [3] solves that stopped at newton_max_iter (the
 *   reference's undefined counterMax, :564)   [4] realisations that left the event loop at max_events
 *   [5] accepted realisations   [6] events at which NO neuron will fire (every candidate time is the "never"
 *   value 100.0f: the block arg-min of :843-881 is then decided by its tie rule)   [7] events at which two
 *   neurons share the minimal REAL firing time (lower bound).
 * Debug only: allocates, synchronises, and costs one more evolve. */
#define MI_EDM_N_COUNTERS 8
mi_status mi_edm_debug_counters(mi_edm* e, uint64_t out[MI_EDM_N_COUNTERS]);
/* duration of the stages of the last compute_f in ms (HIP events):
 * [0] lift, [1] evolve, [2] restrict+mean, [3] whole call */
mi_status mi_edm_last_timings(mi_edm* e, float ms[4]);

/* Test hook: evaluate the device math routines of the pipeline on arrays
 * (op: 0 exp, 1 log, 2 pow(a,b), 3 erfinv; 4: a / b[0] the way the kernels divide
 * by a wave-uniform divisor, 5: a / b[0] by IEEE division; 6..11: the firing test
 * will_fire(v0 = a, s0 = b) -> 0/1 on its exact path (even op) and with its hardware
 * pre-decision (odd op) for beta = 13.0589, 1.5, 0.7; 12: a[i ^ 32], the lane-pair
 * exchange the paired firing-time solves rely on, n a multiple of 64) so that tests can
 * compare them with oracle/edm_oracle.c bit for bit.  Device pointers; b_dev may be NULL. */
mi_status mi_edm_math_probe(mi_ctx* ctx, int math_mode, int op, const float* a_dev, const float* b_dev,
                            float* out_dev, size_t n);

/* ---- several GPUs of one node, one host process ----------------------------
 * The reference is single-GPU (EventDrivenMap.cu:80-94 allocates on the current
 * device, Driver.cu:20 builds one problem); BASELINE configs 4-5 shard the
 * realisation axis -- and the query axis of the table interpolation -- over the
 * GPUs of a node.  A group owns one context (device + stream of
 * its own) per shard.  Host code keeps the reference's shape: ONE ComputeF per
 * residual (AbstractNonlinearProblem.hpp:11, Driver.cu:71) -- see
 * mi_group_edm_compute_f -- and one call per interpolation.
 * devices: ndev ordinals, or NULL for 0..ndev-1.  Naming a device more than once
 * is allowed (rehearsal of the shard arithmetic on a box with fewer GPUs); such a
 * group cannot use RCCL and moves data with device-to-device copies instead. */
typedef struct mi_group mi_group;
typedef struct mi_group_grid1 mi_group_grid1;
typedef struct mi_group_edm mi_group_edm;
mi_status mi_group_create(int ndev, const int* devices, mi_group** out);
mi_status mi_group_destroy(mi_group* g);
int mi_group_size(const mi_group* g);
mi_ctx* mi_group_ctx(mi_group* g, int rank);          /* shard `rank`'s context (owned by the group) */
mi_status mi_group_synchronize(mi_group* g);
/* Member `rank`'s stream waits for the work that `stream` (a hipStream_t of that member's device; NULL: its default stream)
 * holds at the time of the call: an event recorded there, waited for on the device -- the host does not wait (and a
 * stream that is idle at the call costs one hipStreamQuery, no event).  This is how
 * a caller orders the producers of the buffers it hands to mi_group_interp1_f64_dev / mi_group_interp2_f64_dev (and the
 * last writers of the result buffers) in front of the group's kernels; the Python interp_dev forms call it with torch's
 * current stream of every member's device. */
mi_status mi_group_wait_stream(mi_group* g, int rank, void* stream);
/* contiguous, balanced split of n units over `world` shards: shard `rank` = [lo, hi); the first n % world shards get
 * one extra unit.  Host arithmetic only. */
void mi_shard_bounds(size_t n, int rank, int world, size_t* lo, size_t* hi);
/* How mi_group_edm_compute_f adds the shards' partial blocks: on the host, where they already are (default), or with
 * ncclAllReduce on the devices (RCCL over xGMI; distinct devices only). */
#define MI_GROUP_REDUCE_HOST 0
#define MI_GROUP_REDUCE_RCCL 1
mi_status mi_group_set_reduce(mi_group* g, int mode);
/* Number of ranks of the group's RCCL communicator as RCCL reports it (ncclCommCount; the communicator is formed by
 * ncclCommInitAll on first use, here if need be).  0: the group cannot use RCCL (a device named twice, or librccl
 * missing); mi_last_error(NULL) says why.  bench.py --backend group prints it as "rccl_ranks". */
int mi_group_rccl_ranks(mi_group* g);

/* 1-D table replicated on every device of the group (x, y: host pointers; flags as mi_grid1_create). */
mi_status mi_group_grid1_create(mi_group* g, const double* x, const double* y, size_t n, unsigned flags,
                                mi_group_grid1** out);
mi_status mi_group_grid1_destroy(mi_group_grid1* t);
/* Query shards from / to host arrays (the arma::vec-facing form): shard r = mi_shard_bounds(nq, r, P) is uploaded to,
 * evaluated on and downloaded from device r, all shards concurrently; returns when yq is complete. */
mi_status mi_group_interp1_f64_host(mi_group* g, const mi_group_grid1* t, const double* xq, double* yq, size_t nq,
                                    double extrap_val);
/* Device-resident shards: xq_dev[r] / yq_dev[r] point to nq_per_shard doubles on device r.  Asynchronous (each shard on
 * its context's stream; mi_group_synchronize waits).  gathered_dev (optional, may be NULL): gathered_dev[r] is a buffer
 * of P * nq_per_shard doubles on device r that receives EVERY shard's results (shard s at offset s * nq_per_shard;
 * in place when yq_dev[r] == gathered_dev[r] + r * nq_per_shard): an RCCL all-gather over xGMI behind the kernels.
 * The members' streams are not ordered behind any other stream: a C caller orders its own producers with
 * mi_group_wait_stream.  Calls on one group are ordered among themselves, gathers included. */
mi_status mi_group_interp1_f64_dev(mi_group* g, const mi_group_grid1* t, const double* const* xq_dev,
                                   double* const* yq_dev, size_t nq_per_shard, double extrap_val,
                                   double* const* gathered_dev);
/* The gather of mi_group_interp1_f64_dev hidden behind its kernels: chunks >= 2 cuts every shard into that many
 * contiguous chunks, and chunk k is exchanged (grouped ncclBroadcast on a second stream per member) while the kernel of
 * chunk k+1 runs.  1 (default): one kernel per shard, then one ncclAllGather.  Results are identical either way. */
mi_status mi_group_set_gather_chunks(mi_group* g, int chunks);

/* 2-D table (BASELINE.json config 3) replicated on every device of the group; arguments as mi_grid2_create (host
 * pointers), the scattered queries sharded exactly as for the 1-D table. */
typedef struct mi_group_grid2 mi_group_grid2;
mi_status mi_group_grid2_create(mi_group* g, const double* x, size_t nx, const double* y, size_t ny, const double* z,
                                unsigned flags, mi_group_grid2** out);
mi_status mi_group_grid2_destroy(mi_group_grid2* t);
mi_status mi_group_interp2_f64_host(mi_group* g, const mi_group_grid2* t, const double* xq, const double* yq, double* zq,
                                    size_t nq, double extrap_val);
mi_status mi_group_interp2_f64_dev(mi_group* g, const mi_group_grid2* t, const double* const* xq_dev,
                                   const double* const* yq_dev, double* const* zq_dev, size_t nq_per_shard,
                                   double extrap_val, double* const* gathered_dev);
/* Gridded form over the group (mi_interp2_grid_f64_host): member r computes the columns [lo, hi) =
 * mi_shard_bounds(nxi, r, P), one contiguous slice of the column-major zi; yi is replicated.  Synchronous. */
mi_status mi_group_interp2_grid_f64_host(mi_group* g, const mi_group_grid2* t, const double* xi, size_t nxi,
                                         const double* yi, size_t nyi, double* zi, double extrap_val);

/* interp1 over the columns of a matrix, sharded by columns (mi_interp1_cols_f64_host): member r computes the columns
 * [lo, hi) = mi_shard_bounds(ncols, r, P); x (n nodes, validated as by mi_axis1_create) and xi are replicated.  Host
 * pointers, synchronous. */
mi_status mi_group_interp1_cols_f64_host(mi_group* g, const double* x, size_t n, const double* y, size_t ldy, size_t ncols,
                                         const double* xi, size_t nxi, double* yi, size_t ldyi, double extrap_val);

/* interp1 over paired columns, sharded by columns (mi_interp1_pairs_f64_host): member r computes the columns
 * [lo, hi) = mi_shard_bounds(ncols, r, P); xi is replicated.  Host pointers, synchronous; the status rule of
 * mi_interp1_pairs_f64_host (MI_ERR_GRID for a bad column only when col_ok is NULL). */
mi_status mi_group_interp1_pairs_f64_host(mi_group* g, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                          const uint32_t* len, size_t ncols, const double* xi, size_t nxi, double* yi,
                                          size_t ldyi, double extrap_val, uint32_t* col_ok);

/* interp1 over paired columns with a query vector per column, sharded by columns (mi_interp1_each_f64_host): member r
 * computes the columns [lo, hi) = mi_shard_bounds(ncols, r, P); xi is sharded with the columns when ldxi > 0 and
 * replicated when ldxi == 0.  Otherwise as mi_group_interp1_pairs_f64_host. */
mi_status mi_group_interp1_each_f64_host(mi_group* g, const double* x, size_t ldx, const double* y, size_t ldy, size_t n,
                                         const uint32_t* len, size_t ncols, const double* xi, size_t ldxi, size_t nxi,
                                         double* yi, size_t ldyi, double extrap_val, uint32_t* col_ok);

/* EventDrivenMap with the realisations sharded over the group: p->n_real is the TOTAL (>= group size); shard r evolves
 * realisations [lo_r, hi_r) = mi_shard_bounds(n_real, r, P) with real_offset = p->real_offset + lo_r, so the per-neuron
 * draws -- and therefore every result -- are those of the unsharded ensemble. */
mi_status mi_group_edm_create(mi_group* g, const mi_edm_params* p, mi_group_edm** out);
mi_status mi_group_edm_destroy(mi_group_edm* e);
mi_status mi_group_edm_set_params(mi_group_edm* e, const mi_edm_params* p);
/* ComputeF (EventDrivenMap.cu:154-240) over all shards: every device runs lift -> evolve -> restrict -> partial sums
 * concurrently, the partial blocks (MI_EDM_PARTIAL_LEN(n_spikes) doubles per shard) are added (see
 * mi_group_set_reduce) and f is formed from the totals exactly as mi_edm_residual_from_sums does.  z, f: host,
 * n_spikes doubles; partial_total (optional): the summed block. */
mi_status mi_group_edm_compute_f(mi_group_edm* e, const double* z, double* f, double* partial_total);
mi_edm* mi_group_edm_shard(mi_group_edm* e, int rank);               /* shard handle, e.g. for mi_edm_debug_read */
mi_status mi_group_edm_shard_bounds(const mi_group_edm* e, int rank, size_t* lo, size_t* hi);

#ifdef __cplusplus
}
#endif
#endif /* MI355_INTERP_H */
