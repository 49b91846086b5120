/*
 * epgx.h -- C ABI of libepgx.so, the MI355X (gfx950) engine behind epgpy's hot path.
 *
 * The reference (py-baudin/epgpy) has no FFI: its only back-end seam is the array-module
 * switch `set_array_module("cupy")` (epgpy/common.py:21-74).  The boundary this library
 * replaces is therefore the *operator protocol* + `simulate()`:
 *
 *   reference interface (file:line)                     entry point(s) here
 *   --------------------------------------------------  -----------------------------------
 *   functions.simulate / simulate_simple loop           epgx_plan_create + epgx_run
 *     (epgpy/functions.py:50-192)                         (whole sequence or one segment per launch)
 *   DiffOperator.__call__ -> _apply for T/E/P/S         epgx_run on a 1-operator plan
 *     (epgpy/diff.py:119-139, opmatrix.py:199-221,
 *      opscalar.py:213-232, shift.py:82-101,271-294)
 *   StateMatrix storage: states/equilibrium/resize/copy epgx_state_create/upload/download/
 *     (epgpy/statematrix.py:12-80,276-297,654-676)        copy/resize/destroy
 *   Probe.acquire -> asnumpy(F0)  (probe.py:63-66,       signal buffer written by EPGX_OP_ADC,
 *     138-139; statematrix.py:148-175)                    fetched with epgx_memcpy_d2h
 *   cupy device management (common.py:37-47)             epgx_ctx_*, epgx_malloc/free/memcpy
 *
 * Conventions: every function returns EPGX_OK (0) or a negative error code and never throws;
 * epgx_last_error() returns a thread-local message for the last failure on this thread.
 * The caller owns all host buffers; the library owns device buffers it allocates.  All work
 * is enqueued on the context's HIP stream (own stream, or one adopted with
 * epgx_ctx_set_stream); host copies synchronise that stream.  One context per (thread, device).
 * There is NO CPU fallback: with no usable GPU epgx_ctx_create fails with EPGX_ERR_NODEVICE.
 *
 * Data layouts (all complex128 = 2 x float64 interleaved):
 *   state  : [nvox][3][K]  half representation, order k = 0..K-1 contiguous,
 *            comp 0 = F_k, comp 1 = conj(F_-k), comp 2 = Z_k   (reference: [*grid, 2n+1, 3],
 *            statematrix.py:55; the k<0 rows are the mirror image, statematrix.py:416-421)
 *   density: [nvox] float64, equilibrium magnetisation (statematrix.py:379-385)
 *   signal : [n_adc][signal_ld] complex128, slot-major ("(n_adc, *grid)", functions.py:157-165); entry points that hand
 *            records to the HOST take an epgx_signal_dtype: EPGX_SIGNAL_C64 rounds every record once, on the device, to
 *            2 x float32 before it crosses PCIe (the arithmetic and the device-side records stay complex128)
 *
 * The operator stream is given as primitives (one epgx_op per reference operator); the library
 * packs them into fused [T][E][S][ADC] records internally ("S E" is emitted as "E S", which is
 * bit-identical because E multiplies every order by the same factors and S only moves values).
 */
#ifndef EPGX_H
#define EPGX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPGX_ABI_VERSION 11
#define EPGX_MAX_DIMS 8    /* grid dimensions                        */
#define EPGX_MAX_SPACES 4  /* distinct operator broadcast patterns   */
#define EPGX_WAVE 64       /* k-states per lane-register (wave64)    */
#define EPGX_MAX_K 2048    /* max k-states per voxel: 1024 for states in HBM (16 per lane), 2048 state-resident */
#define EPGX_MAX_VARS 3    /* derivative variables carried per launch */

enum epgx_status {
    EPGX_OK = 0,
    EPGX_ERR_INVALID = -1,     /* bad argument / inconsistent plan            */
    EPGX_ERR_HIP = -2,         /* a HIP runtime call failed                   */
    EPGX_ERR_NOMEM = -3,       /* device or host allocation failed            */
    EPGX_ERR_UNSUPPORTED = -4, /* valid request the kernels do not cover      */
    EPGX_ERR_NODEVICE = -5     /* no MI355X-class device visible              */
};

/* Operator stream.  Coefficients live in one float64 pool; an operator with coefficients
 * reads `ncoef` doubles at  pool[coef_off + index(space, voxel) * ncoef]. */
enum epgx_opcode {
    EPGX_OP_NOP = 0,
    EPGX_OP_T = 1,     /* RF rotation, 8 coef: m00, Re/Im m01, Re/Im m02, Re/Im m20, m22
                          (m00, m22 real; m10=conj m01, m11=m00, m12=conj m02, m21=conj m20)
                          -- transition.py:114-151                                           */
    EPGX_OP_MAT = 2,   /* general symmetric 3x3, 9 coef: Re/Im m00, Re/Im m01, Re/Im m02,
                          Re/Im m20, m22 (m11 = conj m00) -- opmatrix.py:157-170             */
    EPGX_OP_E = 3,     /* diagonal, 4 coef: Re/Im e0 (multiplies F_k; conj(e0) multiplies
                          col 1), e2 (Z), r0 (Z_0 += r0*density) -- evolution.py:220-256      */
    EPGX_OP_S = 4,     /* integer shift by ia (!= 0) with truncation at K -- shift.py:271-294 */
    EPGX_OP_ADC = 5,   /* signal[ia] <- F0 (ib = 0) or Z0 (ib = 1) -- statematrix.py:148-175  */
    EPGX_OP_SPOIL = 6, /* F <- 0 -- operator.py:281-286                                      */
    EPGX_OP_RESET = 7, /* state <- equilibrium -- operator.py:297-304                        */
    EPGX_OP_PD = 8,    /* density <- coef[0]; ia != 0: state <- new equilibrium
                          -- operator.py:315-341                                             */
    EPGX_OP_D = 9,     /* per-order real diagonal, ncoef = 3*K doubles per entry laid out [3][K]:
                          F_k *= c[0][k], conj(F_-k) *= c[1][k], Z_k *= c[2][k]
                          -- diffusion.py:60-79 (D operator; the table is built on the host from the
                          k-space coordinates and the diffusion coefficient / tensor)             */
    EPGX_OP_GS = 10,   /* host-planned gather shift, ncoef = 3*K/2 doubles = int32 [3][K]: for each
                          new order the old order its F / conj(F-) / Z comes from; -1 = zero,
                          index | 1<<30 = conjugate of the partner array -- shift.py:297-364 (shiftnd) */
    EPGX_OP_MAT0 = 11, /* EPGX_OP_MAT plus a constant term, 14 coef: the 10 of MAT, then Re/Im o0, o2, pad:
                          (o0, conj o0, o2) * density is added to (F_0, conj F_0, Z_0) -- the effect of
                          `mat0 @ equilibrium` (opmatrix.py:199-205); produced by `E @ T` combinations, and by
                          the library itself for a collapsed run of operators (epgx_chain)            */
    EPGX_OP_T0 = 12,   /* EPGX_OP_T plus a constant term, 12 coef: the 8 of T, then Re/Im o0, o2, pad.  What a
                          T between two precession-free relaxations collapses to: E2 T E1 keeps T's
                          symmetry and real m00 (the diagonal of E is real), and the recoveries become
                          (o0, conj o0, o2) * density on the k = 0 order.  Emitted by the host's
                          peephole fusion (epgpy_amd/fusion.py); same idea as `E @ T` in the reference */
    EPGX_OP_X = 13,    /* exchange between the N = ia (2 .. 8) compartments of a voxel group -- exchange.py:89-120, 154-207.
                          The compartments of a group are the voxels v, v + ib, .., v + (N-1) ib of the grid (ib = the
                          compartment stride in voxels: the product of the grid extents behind the compartment axis).  One
                          table entry per GROUP (an index space with stride 0 on the compartment axis, evaluated at any of
                          its voxels), 3 N^2 doubles: Re/Im of mT row-major (2 N^2), then mL row-major (N^2).  mL is stored
                          real: the reference's expm of a real matrix carries an imaginary part that is rounding noise of
                          its eigendecomposition.  At every order k, with rho_c the density of compartment c:
                            A_c <- sum_c' mT[c][c'] A_c'                (A = F_k)
                            B_c <- sum_c' conj(mT[c][c']) B_c'          (B = conj F_-k)
                            Z_c <- sum_c' mL[c][c'] (Z_c' - d_k0 rho_c') + d_k0 rho_c
                          A range that holds X runs in ONE launch of xrun_kernel<NC, M, HAS_IN> (NC = N = 2 .. 4, K / 64 = M
                          with NC M <= 8, no D / gather shifts; one wavefront per group, the state in registers); otherwise
                          (or with EPGX_XRUN=0 in the environment) as pieces: the records between two X on the per-timestep
                          kernels with the state in HBM (a temporary state from equilibrium when `in` is NULL),
                          exchange_kernel in between.  epgx_kernel_for names the first "xrun_kernel<2, 2, false>" (etc.),
                          the second "split<exchange_kernel>".  Voxel ranges must hold whole groups.
                          With derivative states (n_vars > 0) X is a DIFFERENTIABLE operator, not a plain one: it always acts on
                          the derivative states, independent of EPGX_DERIV_THROUGH_PLAIN_OPS, and may carry partials (epgx_dop).
                          At every order k, the partial terms reading the state BEFORE its update:
                            dA_v,c <- sum_c' mT[c][c'] dA_v,c'       + sum_c' dmT_v[c][c'] A_c'
                            dB_v,c <- sum_c' conj(mT[c][c']) dB_v,c' + sum_c' conj(dmT_v[c][c']) B_c'
                            dZ_v,c <- sum_c' mL[c][c'] dZ_v,c'       + sum_c' dmL_v[c][c'] (Z_c' - d_k0 rho_c')
                          (no equilibrium term in the derivative states; the densities depend on no variable).  Such a range runs in
                          ONE launch of dxrun_kernel<NC, M, V> (V = n_vars): NC = 2 .. 4 with NC M (1 + V) <= 8, state-resident
                          from equilibrium (in = out = NULL), no D / gather shifts, first order; everything else is
                          EPGX_ERR_UNSUPPORTED -- there is no split path for derivatives.  A plan that holds X and variables keeps
                          every relaxation a stage of its own: a generated EPGX_OP_T0 partial (epgx_fuse_partial) is refused. */
    EPGX_OP__COUNT
};

typedef struct epgx_op {
    int32_t opcode;   /* enum epgx_opcode                                  */
    int32_t space;    /* index space of the coefficient table, or -1       */
    int32_t ia;       /* S: shift; ADC: output slot; PD: reset flag        */
    int32_t ib;       /* ADC: 0 = F0, 1 = Z0                               */
    int64_t coef_off; /* first double of this operator's table in the pool */
    int32_t ncoef;    /* doubles per table entry                           */
    int32_t reserved;
} epgx_op; /* 32 bytes */

/* First-order partial derivatives of operator i w.r.t. up to EPGX_MAX_VARS variables
 * (DiffOperator order1, epgpy/diff.py:264-288).  coef_off[v] < 0: operator i does not depend on
 * variable v.  Table entry: EPGX_OP_T / MAT / MAT0 -> the 10 coefficients of EPGX_OP_MAT for
 * d(mat)/dv;  EPGX_OP_E -> 4 coefficients (Re/Im d e0, d e2, d r0) for d(arr, arr0)/dv;  EPGX_OP_X -> a table in the
 * layout of X's own, one entry per compartment group of 3 N^2 doubles (Re/Im of d mT / dv row-major, then d mL / dv, real); already
 * combined over the operator's parameters (sum_p coeff[v][p] * dOp/dp).  An EPGX_OP_T0 whose table the library
 * generated (epgx_fuse) takes its partials from tables the library generates as well (epgx_fuse_partial: coef_off in
 * the generated part of the pool, 14 per entry -- the 10 of d(mat)/dv, then Re/Im d o0, d o2, pad).  A partial table may
 * also be one the library ASSEMBLES from per-axis columns (epgx_assemble: d(relaxation)/dT2 over a (T1, T2) grid varies with
 * T2 only): coef_off then names the recipe's destination. */
typedef struct epgx_dop {
    int32_t space[EPGX_MAX_VARS]; /* index space of the partial's table, or -1 */
    int32_t reserved;             /* 0; under EPGX_DERIV_SECOND: EPGX_HESS_CROSS_* bits of this operator  */
    int64_t coef_off[EPGX_MAX_VARS];
} epgx_dop; /* 40 bytes */

/* A table that the LIBRARY generates on the device when the plan is created: the EPGX_OP_T0 table
 * of "T sandwiched with a precession-free E" (see EPGX_OP_T0).  Sources are tables of the pool (host
 * part, or tables generated by earlier entries of the list); the destination lies in the generated
 * part of the pool, [n_coef, n_coef + n_coef_generated).  Every index space that a source varies
 * along must be one the destination varies along.  (The host would need ~0.1 s of NumPy per
 * 1024 x 1024 table; the device writes it in ~0.1 ms.) */
typedef struct epgx_fuse {
    int64_t dst_off;   /* doubles, in the generated part; 12 coefficients per entry (EPGX_OP_T0 layout) */
    int64_t src_off;   /* the rotation: EPGX_OP_T layout (8 per entry) or EPGX_OP_T0 layout (12)          */
    int64_t e_off;     /* the relaxation: EPGX_OP_E layout, Im e0 = 0 in every entry                       */
    int32_t dst_space, src_space, e_space; /* index spaces (-1: one entry for all voxels)                */
    int32_t src_ncoef; /* 8 or 12                                                                          */
    int32_t after;     /* 1: E acts after the rotation (rows scaled), 0: before it (columns scaled)        */
    int32_t reserved;
} epgx_fuse; /* 48 bytes */

/* The partial derivative of an epgx_fuse table with respect to one variable, generated next to it (product rule:
 * d(E T) = dE T + E dT, the constant term likewise).  A differentiated  E . T . E  sandwich then costs the kernels one
 * rotation per state and one accumulation per derivative state instead of three stages each (the 20-echo 1024 x 1024
 * Jacobian with one variable: 66 -> 46 fp64 instructions per order and echo).  Sources: the operands of the epgx_fuse
 * entry that produced the value table, and their partials -- a rotation partial in the host part of the pool (10 per
 * entry, epgx_dop layout), or one generated by an EARLIER entry of this list (14 per entry), or none (-1); a
 * relaxation partial (4 per entry, Im d e0 = 0 in every entry; in the host part of the pool or an assembled table) or none.
 * At least one of the two must be given.
 * Executed after the `fuse` list, in order. */
typedef struct epgx_fuse_partial {
    int64_t dst_off;   /* doubles, in the generated part; 14 per entry: d(mat)/dv (10), Re/Im d o0, d o2, pad      */
    int64_t src_off;   /* the rotation's VALUE table, as in the epgx_fuse entry (8 or 12 per entry)                  */
    int64_t dsrc_off;  /* its partial, or -1                                                                          */
    int64_t e_off;     /* the relaxation's VALUE table (4 per entry)                                                  */
    int64_t de_off;    /* its partial, or -1                                                                          */
    int32_t dst_space, src_space, dsrc_space, e_space, de_space;   /* index spaces (-1: one entry for all voxels)   */
    int32_t src_ncoef; /* 8 or 12                                                                                     */
    int32_t dsrc_ncoef;/* 10 or 14 (ignored when dsrc_off < 0)                                                        */
    int32_t after;     /* as in epgx_fuse                                                                              */
} epgx_fuse_partial; /* 72 bytes */

/* A table that the library ASSEMBLES on the device from per-axis columns when the plan is created.  The
 * reference builds e.g. the relaxation table of E(tau, T1[:, None], T2[None, :]) by evaluating exp() on the
 * un-broadcast parameter arrays and broadcasting the results into [*grid, 3] (evolution.py:220-242): the table is an
 * outer combination of a few small columns.  Shipping the columns (2 x 1024 x 2 doubles) and letting the device write
 * the 1024 x 1024 x 4 table (34 MB in ~10 us) replaces packing and uploading the full table on every simulate()
 * (~5 ms) -- with the SAME bits, because the column values are the reference's own.
 *   destination column c of entry i  =  coef[src[col_src[c]].off + index_i(src[col_src[c]].strides) * ncol + col_idx[c]]
 * Sources lie in the host part of the pool; the destination in the generated part (like epgx_fuse, whose sources
 * may be assembled tables: the list is executed before the fuse list).  Every axis a source varies along must be
 * one the destination's index space varies along. */
#define EPGX_MAX_ASM_SRC 4
#define EPGX_MAX_ASM_COLS 16
typedef struct epgx_asm_src {
    int64_t off;                     /* first double of the source columns: [entries][ncol]        */
    int32_t ncol, reserved;
    int64_t strides[EPGX_MAX_DIMS];  /* entry index = sum_d coord[d] * strides[d]                   */
} epgx_asm_src; /* 80 bytes */
typedef struct epgx_assemble {
    int64_t dst_off;                 /* doubles, in the generated part; ncoef per entry             */
    int32_t dst_space, ncoef;        /* ncoef <= EPGX_MAX_ASM_COLS                                  */
    int32_t n_src, reserved;
    epgx_asm_src src[EPGX_MAX_ASM_SRC];
    uint8_t col_src[EPGX_MAX_ASM_COLS], col_idx[EPGX_MAX_ASM_COLS];
} epgx_assemble; /* 376 bytes */

/* A table that the library COLLAPSES on the device when the plan is created: the affine map of a run of state-wise operators
 * that holds no shift and no probe -- a sampled RF pulse (rfpulse.py: N small rotations with relaxation / precession in
 * between, 2 N to 3 N operators) is the same map (M, o) at every order of a voxel, so it is multiplied up ONCE per table entry
 * and applied as one EPGX_OP_MAT0 record (chain_kernel, csrc/epgx_chain.hip: one lane per destination entry, the running map
 * in registers, every step a left-multiplication (M, o) <- (A M, A o + a)).
 * A step names a source table of the pool by the opcode whose layout it has: EPGX_OP_T (8 per entry), EPGX_OP_MAT (10),
 * EPGX_OP_MAT0 (14) or EPGX_OP_E (4, e0 complex: precession allowed).  Steps come in GROUPS that are repeated: the `group`
 * steps from a group's first step on are executed `count` times in order, repetition r reading the table at off + r * stride
 * -- the N rotation tables of a pulse lie one after the other in the pool and share one relaxation table, so a whole pulse is
 * one group {T: stride = one table, E: stride 0} with count = N.  `count` / `group` are read from the first step of a group
 * (0 in the others); a group has at most EPGX_CHAIN_GROUP steps.
 * Sources lie in the host part of the pool or are assembled tables (the list is executed after `assemble` and before `fuse`);
 * the destination lies in the generated part, 14 per entry (EPGX_OP_MAT0 layout).  Every axis a source varies along must be
 * one the destination varies along. */
#define EPGX_CHAIN_GROUP 4
typedef struct epgx_chain_step {
    int64_t off;     /* first double of the source table (of repetition 0)                              */
    int64_t stride;  /* doubles from the table of one repetition to that of the next (0: the same table) */
    int32_t kind;    /* EPGX_OP_T, EPGX_OP_MAT, EPGX_OP_MAT0 or EPGX_OP_E                                */
    int32_t space;   /* index space of the source (-1: one entry for all voxels)                         */
    int32_t count;   /* first step of a group: repetitions (>= 1)                                        */
    int32_t group;   /* first step of a group: steps in the group (1 .. EPGX_CHAIN_GROUP)                */
} epgx_chain_step; /* 32 bytes */
typedef struct epgx_chain {
    int64_t dst_off;              /* doubles, in the generated part; 14 coefficients per entry          */
    int32_t dst_space;            /* index space of the destination (-1: one entry)                     */
    int32_t n_steps;
    const epgx_chain_step *steps; /* [n_steps]                                                          */
} epgx_chain; /* 24 bytes */

/* What epgx_plan_desc cannot take up without changing its size: passed to epgx_plan_create_ext next to it.  Set
 * struct_size = sizeof(epgx_plan_ext) and zero every member you do not use. */
typedef struct epgx_plan_ext {
    uint32_t struct_size;
    int32_t n_chain;              /* device-collapsed tables (executed after `assemble`, before `fuse`)  */
    const epgx_chain *chain;      /* [n_chain]                                                           */
} epgx_plan_ext; /* 16 bytes */

/* Host-side description of a compiled sequence ("plan").  The parameter grid has `ndim`
 * axes of extent grid_shape[d] (C order, last axis fastest); voxel v has coordinates
 * unravel(v).  Index space s maps a voxel to  sum_d coord[d] * space_strides[s][d]
 * (stride 0 on axes the operator does not depend on: the reference's append-trailing-axes
 * broadcasting, common.py:273-303).  Set struct_size = sizeof(epgx_plan_desc) and zero every member you do not use. */
typedef struct epgx_plan_desc {
    uint32_t struct_size;         /* sizeof(epgx_plan_desc) of the header the CALLER was built against: epgx_plan_create
                                     rejects any other value with EPGX_ERR_INVALID instead of reading past a shorter struct */
    int32_t n_ops;
    const epgx_op *ops;
    int32_t ndim;
    const int64_t *grid_shape;    /* [ndim]                       */
    int32_t n_spaces;
    const int64_t *space_strides; /* [n_spaces][EPGX_MAX_DIMS]    */
    int64_t n_coef;
    const double *coef;           /* [n_coef]                     */
    int32_t n_adc;                /* number of signal slots (rows of the signal buffer)           */
    int32_t n_vars;               /* 0, or 1..EPGX_MAX_VARS: run with first-order derivatives; every
                                     ADC then writes 1 + n_vars consecutive rows starting at its
                                     slot: the probe of the state, then of each derivative state      */
    const epgx_dop *dops;         /* [n_ops] when n_vars > 0, else NULL                               */
    int32_t deriv_flags;          /* EPGX_DERIV_*                                                      */
    int32_t n_fuse;               /* device-generated tables                                           */
    const epgx_fuse *fuse;        /* [n_fuse], executed in order                                        */
    int64_t n_coef_generated;     /* doubles appended to the pool for them (operators may refer to
                                     offsets up to n_coef + n_coef_generated)                          */
    int32_t n_assemble;           /* device-assembled tables (executed before `fuse`)                  */
    int32_t n_fuse_partial;       /* partials of device-generated tables (executed after `fuse`)       */
    const epgx_assemble *assemble;/* [n_assemble]                                                      */
    const epgx_fuse_partial *fuse_partial; /* [n_fuse_partial]                                         */
} epgx_plan_desc;

/* The reference propagates derivative states through its DiffOperators only (T/MAT, E, S);
 * SPOIL, RESET, PD and D are plain Operators there and leave sm.order1 untouched
 * (epgpy/operator.py:95-104 vs epgpy/diff.py:119-139), e.g. the "derivative" of a spoiled signal
 * stays non-zero.  Default (flag clear): the same for SPOIL and D, for identical numbers.  Flag
 * set: these operators, which are linear and independent of the variables, act on the derivative
 * states too (d(Op S)/dv = Op dS/dv), which is the derivative of the signal that is actually
 * simulated.  A reset (RESET, PD with reset) always clears the derivative states: the reference
 * keeps stale ones of the old size there and then NumPy-broadcasts a 1-row partial over them. */
#define EPGX_DERIV_THROUGH_PLAIN_OPS 1
/* Also carried in `deriv_flags`: keep every relaxation a stage of its own.  By default the library folds
 * precession-free relaxations (EPGX_OP_E with Im e0 = 0) into a neighbouring rotation whenever their tables
 * cannot be multiplied ahead of time (different index spaces): the wavefront then computes the coefficients of
 * E_after . T . E_before for its voxels at run time -- rounding-level differences to the operator-by-operator
 * product, as with EPGX_OP_T0 tables.  The fold is a property of the plan (every launch of it, at every capacity,
 * runs the same chains -- the same bits, up to the sum / difference form of rotations about x in the 64-order state-resident
 * kernels, see epgx_run); the host sets this flag for `simulate(fuse=False)` and for plans it runs with 16 orders
 * per voxel (one order per lane: a relaxation stage is then cheaper than the fold's extra loads).
 * Plans WITH derivative states fold as well, for state-resident launches at 64 orders whose records are mostly runs of one
 * repetition shape: the relaxations' partials then enter through their logarithmic form (a real relaxation's partial is a
 * multiple of the relaxation: the library derives (d e / e, d e2 / e2) per table entry on the device when the plan is
 * created and checks d r = -d e2), the rotation's partial is folded like the rotation.  The same route serves the
 * relaxation-only partials of epgx_fuse_partial tables inside runs.  Results equal the unfolded recurrence to rounding;
 * this flag switches all of it off. */
#define EPGX_PLAN_NO_FOLD 2
/* Also carried in `deriv_flags`: the plan is a ONE-PAIR SECOND-ORDER PASS for the variable pair (a, b)
 * (DiffOperator order2, epgpy/diff.py:290-379).  Per operator:
 *     H_ab <- Op H_ab + (dOp/da) S_b + (dOp/db) S_a + (d2Op/da db) S,   S_a, S_b, S as in a first-order plan.
 * n_vars = 3 (a != b): slots 0 and 1 of every epgx_dop hold dOp/da and dOp/db, slot 2 the COMBINED second-order table
 *     sum_p order2[pair][p] dOp/dp + sum_{p1, p2} c1 c2 d2Op/dp1 dp2   (same layouts as the first-order tables; combined
 * on the host), acting on S (with its recovery term); every ADC writes four rows: the probe of S, S_a, S_b, H_ab.
 * n_vars = 2 (a == b): slot 0 holds dOp/da, slot 1 the combined second-order table, the cross term is 2 (dOp/da) S_a;
 * every ADC writes three rows: S, S_a, H_aa.
 * Which cross terms enter at an operator is the HOST's decision (the reference takes a cross term only when the pair is in the
 * operator's order2 or, with auto_cross_derivatives, when the other variable is alive in the state): epgx_dop::reserved
 * carries EPGX_HESS_CROSS_A (the term (dOp/da) S_b; for a == b the doubled term) and EPGX_HESS_CROSS_B ((dOp/db) S_a);
 * a cross bit whose first-order slot is empty is EPGX_ERR_INVALID.  The second-order term enters where its slot is filled.
 * Plain operators act on H as on the first-order states (EPGX_DERIV_THROUGH_PLAIN_OPS); a reset clears H.
 * Such a plan must set EPGX_PLAN_NO_FOLD and may not carry device-generated tables (n_fuse, n_fuse_partial) or chains: the
 * run-time fold and epgx_fuse_partial implement the first-order product rule only (EPGX_ERR_UNSUPPORTED).  It runs
 * state-resident from equilibrium on hess_kernel<K / 64, NSP, a == b> at K = 64, 128, 256, 512 (EPGX_ERR_UNSUPPORTED otherwise). */
#define EPGX_DERIV_SECOND 4
#define EPGX_HESS_CROSS_A 1
#define EPGX_HESS_CROSS_B 2

/* Record type of HOST-side signal arrays (and of narrowed device buffers, epgx_signal_narrow).  The reference returns
 * complex128 (statematrix.py:392); complex64 halves what crosses PCIe / xGMI -- the part of a large simulate() its caller
 * actually waits for -- at one rounding per record (<= 6e-8 relative, inside the 1e-6 parity bar). */
enum epgx_signal_dtype {
    EPGX_SIGNAL_C128 = 0, /* 2 x float64 (default everywhere) */
    EPGX_SIGNAL_C64 = 1   /* 2 x float32                      */
};

typedef struct epgx_device_info {
    char name[128];
    char arch[64];
    int32_t compute_units;
    int32_t wavefront_size;
    int32_t clock_khz;
    int32_t reserved;
    int64_t hbm_bytes;
} epgx_device_info;

typedef struct epgx_ctx epgx_ctx;
typedef struct epgx_plan epgx_plan;
typedef struct epgx_state epgx_state;

/* ---- library / context -------------------------------------------------------------- */
int epgx_abi_version(void);
const char *epgx_last_error(void);
int epgx_device_count(void);
int epgx_ctx_create(int device, epgx_ctx **out);
int epgx_ctx_destroy(epgx_ctx *ctx);
int epgx_ctx_set_stream(epgx_ctx *ctx, void *hip_stream); /* adopt an external hipStream_t (NULL: own) */
int epgx_ctx_synchronize(epgx_ctx *ctx);
int epgx_ctx_info(epgx_ctx *ctx, epgx_device_info *out);
/* Device blocks freed through this library (epgx_free, plan / state destroy) are cached in the
 * context and recycled (stream-ordered, no device synchronisation); this returns them to HIP. */
int epgx_ctx_release_cache(epgx_ctx *ctx);

/* ---- raw device memory (replaces cupy's allocator for this path) --------------------- */
int epgx_malloc(epgx_ctx *ctx, int64_t bytes, void **dptr);
int epgx_free(epgx_ctx *ctx, void *dptr);
int epgx_memset(epgx_ctx *ctx, void *dptr, int value, int64_t bytes);
int epgx_memcpy_h2d(epgx_ctx *ctx, void *dptr, const void *host, int64_t bytes);
int epgx_memcpy_d2h(epgx_ctx *ctx, void *host, const void *dptr, int64_t bytes);
int epgx_memcpy_d2d(epgx_ctx *ctx, void *dst, const void *src, int64_t bytes);

/* Page-locked host memory, cached in the context like device blocks (pinning 336 MB costs tens of ms; a result
 * array that lives in a recycled pinned block receives its D2H copy at the full PCIe rate, asynchronously). */
int epgx_host_alloc(epgx_ctx *ctx, int64_t bytes, int32_t cached_only, void **hptr); /* cached_only != 0: hand out a recycled
                                                     block or *hptr = NULL (EPGX_OK either way), never pin new memory */
int epgx_host_free(epgx_ctx *ctx, void *hptr);
/* Page-lock memory the CALLER owns (hipHostRegister) -- e.g. a mapping of a shared-memory result that several rank
 * processes fill, each over its own PCIe link (epgpy_amd.distributed.SharedResult): copies into registered memory are
 * direct DMA, like copies into epgx_host_alloc blocks.  Unregister before the memory is unmapped or freed. */
int epgx_host_register(epgx_ctx *ctx, void *hptr, int64_t bytes);
int epgx_host_unregister(epgx_ctx *ctx, void *hptr);

/* ---- timing on the context's stream (HIP events) -------------------------------------- */
int epgx_timer_start(epgx_ctx *ctx);
int epgx_timer_stop(epgx_ctx *ctx, float *elapsed_ms); /* synchronises */

/* ---- plan ---------------------------------------------------------------------------- */
int epgx_plan_create(epgx_ctx *ctx, const epgx_plan_desc *desc, epgx_plan **out);
/* The same with the lists of an epgx_plan_ext next to the description; ext = NULL: none.  EPGX_ERR_INVALID with epgx_last_error() text for a chain whose
 * offsets leave the pool, whose destination is not in the generated part, with an unknown kind, a malformed group, or a
 * source that varies along an axis the destination does not. */
int epgx_plan_create_ext(epgx_ctx *ctx, const epgx_plan_desc *desc, const epgx_plan_ext *ext, epgx_plan **out);
int epgx_plan_destroy(epgx_plan *plan);

/* ---- state (device-resident StateMatrix storage) -------------------------------------- */
int epgx_state_create(epgx_ctx *ctx, int64_t nvox, int32_t K, epgx_state **out); /* equilibrium, density 1 */
int epgx_state_destroy(epgx_state *st);
int epgx_state_upload(epgx_state *st, const double *half /*[nvox][3][K] c128*/,
                      const double *density /*[nvox] or NULL*/);
int epgx_state_download(const epgx_state *st, double *half, double *density /*nullable*/);
int epgx_state_copy(epgx_state *dst, const epgx_state *src); /* same nvox; K may differ (zero pad / truncate) */
int epgx_state_broadcast(epgx_state *dst, const epgx_state *src, const int32_t *src_index /*[dst nvox], host*/);
int epgx_state_info(const epgx_state *st, int64_t *nvox, int32_t *K, void **data, void **density);
/* dst += alpha * src (same nvox and K); zero_density != 0 also clears dst's density, which makes dst
 * a derivative state (no equilibrium term: DiffOperator.derive1, epgpy/diff.py:103-109). Replaces
 * StateMatrix.__iadd__ in diff.accumulate (epgpy/diff.py:553-563) for operator-by-operator use. */
int epgx_state_axpy(epgx_state *dst, const epgx_state *src, double alpha, int32_t zero_density);

/* Spatial read-out of a device-resident state matrix: what DFT / Imaging compute on downloaded arrays in the reference
 * (epgpy/probe.py:168-219 -> epgpy/utils.py:12-115 `imaging` / `_dft`),
 *   out[v][p] = phase * sum_r  w_r F_r(v) exp(i k_r . x_p),        v = vox0 .. vox0 + nvox - 1,  p = 0 .. npos - 1
 * r over the 2 nrow - 1 rows of the state matrix.  Row -k is the mirror image of stored order j (comp 1 = conj(F_-k)), carries
 * the wavenumber -k_j and the same voxel factor, so the sum is taken over the nrow STORED orders (csrc/epgx_dft.hip).
 *   nrow : stored orders used, nstate + 1 (1 .. K of the state); order 0 is k = 0
 *   k    : host [nrow][d], wavenumber of stored order j in rad/m (StateMatrix.k: integer coordinate x kvalue), the columns
 *          that enter the phase
 *   w    : host [nrow], voxel factor of stored order j: 1 for a point, prod_d sinc(k_d size_d / 2 pi) for a box (over ALL
 *          wavenumber columns), 0 for an order the caller drops (utils.py:55-57 `kmask`)
 *   pos  : host [npos][d], d = 1 .. 3
 *   phase_re / phase_im : exp(i phase), multiplies every output (utils.py:78-79); (1, 0) for none
 *   out  : DEVICE, [nvox][npos] complex128.  Weights and sums over axes of this record: epgx_signal_reduce with ONE row whose
 *          grid is (*grid, *positions).
 * Coordinates that differ between voxel classes (a vectorised shift; a class is a contiguous voxel range): one call per class.
 * sin / cos are evaluated in full double precision.  Stream-ordered behind the operators that produced the state; the call
 * uploads k, w and pos (and synchronises for that) before it launches.
 * Errors (nothing is launched): EPGX_ERR_INVALID for a NULL argument, a state of another context, nrow outside [1, K], d outside
 * [1, 3], a voxel range outside the state, npos < 1; EPGX_ERR_UNSUPPORTED when the coefficient table of the call (32 bytes per
 * voxel and order) would exceed 8 GiB or the range 65535 x 256 voxels: hand over voxel slabs. */
int epgx_state_dft(epgx_ctx *ctx, const epgx_state *st, int64_t vox0, int64_t nvox, int32_t nrow, const double *k,
                   const double *w, int32_t d, const double *pos, int64_t npos, double phase_re, double phase_im, void *out);

/* The two device primitives of the float-wavenumber shift (epgpy/shift.py:367-449 `shiftmerge`; csrc/epgx_merge.hip).  The
 * host plans the new row structure from the coordinates alone (epgpy_amd/kmerge.py); what depends on the state -- the weights
 * of the merged coordinates and the pruning test -- comes from epgx_state_row_stats, the scatter-add of several old rows into
 * one new row from epgx_state_merge.  Both are stream-ordered behind the operators that produced the state and validate
 * before anything is launched.
 *
 * epgx_state_row_stats: for every stored order j < nrow, over ALL voxels v of the state,
 *   sums[c * nrow + j] = sum_v |comp_c,j(v)|,  c = 0, 1, 2   (complex moduli of F_j, conj(F_-j), Z_j)
 *   maxabs[j]          = max_v max_c |comp_c,j(v)|
 * (row -j of the reference layout holds the conjugates of stored order j, so its moduli are these with c = 0 and 1 swapped).
 * A modulus is sqrt(re re + im im), every operation rounded on its own.  Deterministic: the association order of every sum
 * depends on nvox alone (no atomics), two calls on equal states return equal bits.  sums / maxabs are HOST arrays; the call
 * synchronises the context's stream.  Errors: EPGX_ERR_INVALID for a NULL argument, a state of another context, nrow outside
 * [1, K]. */
int epgx_state_row_stats(epgx_ctx *ctx, const epgx_state *st, int32_t nrow, double *sums /*[3][nrow]*/, double *maxabs /*[nrow]*/);

/* epgx_state_merge: the multi-source gather, for every voxel v, component c and order j of dst,
 *   dst[v][c][j] = sum over s in [offsets[c][j], offsets[c][j + 1]) of  src[v][comp(e_s)][order(e_s)]  or its conjugate,
 *   e_s = sources[s] = order | comp << 16 | (1 << 30 if conjugated: the flag of EPGX_OP_GS)
 * added in the order listed, starting from +0 (the bits of NumPy's add.at on zeros); an empty list and every order from
 * nrow_dst on give exact zero.  offsets is host int32 [3][nrow_dst + 1] in CSR form over ONE list: offsets[0][0] = 0,
 * non-decreasing, offsets[c + 1][0] = offsets[c][nrow_dst]; sources has offsets[2][nrow_dst] entries.  dst and src are
 * different states of the same context and number of voxels; their capacities may differ.  dst takes the densities of src.
 * The call uploads the table (and synchronises for that) before it launches.
 * Errors (nothing is launched): EPGX_ERR_UNSUPPORTED for nrow_dst > 1024 (checked first); EPGX_ERR_INVALID for a NULL
 * argument, states of another context, dst == src, different nvox, nrow_dst outside [1, K of dst], a table that is not in
 * CSR form, a source entry with a component above 2, an order outside the source's capacity or unknown bits. */
int epgx_state_merge(epgx_ctx *ctx, epgx_state *dst, const epgx_state *src, int32_t nrow_dst, const int32_t *offsets,
                     const int32_t *sources);

/* The per-voxel float shift (epgpy/shift.py:478-629 `shiftprune`; csrc/epgx_prune.hip): a float wavenumber that varies along
 * a grid axis gives every voxel its own coordinate set.  An epgx_coords buffer holds, next to a state of 64 stored orders,
 * the coordinates [nvox][kdim][64] (float64, stored order j of voxel v in column c at k[(v * kdim + c) * 64 + j]) and the
 * number of live stored rows per voxel; rows from the live count on are exact zeros in state and coordinates.
 *
 * epgx_coords_create: all coordinates zero, live counts zero (to be filled by upload, widen or a shift).
 * epgx_coords_upload: host k [nsrc][kdim][64] and nlive [nsrc] (each in [1, 64]); nsrc = nvox, or 1: the one set is repeated
 *   for every voxel on the device.  epgx_coords_download: the reverse, always [nvox].
 * epgx_coords_widen: dst (kdim >= that of src, same nvox) takes the coordinates of src, further columns zero.
 * Errors: EPGX_ERR_INVALID for a NULL argument, nvox < 1, kdim outside 1 .. 4, nsrc other than 1 or nvox, a live count outside
 * [1, 64], buffers of different contexts or sizes.  (`struct epgx_coords` is opaque like the other handles.) */
int epgx_coords_create(epgx_ctx *ctx, int64_t nvox, int32_t kdim, struct epgx_coords **out);
int epgx_coords_destroy(struct epgx_coords *c);
int epgx_coords_info(const struct epgx_coords *c, int64_t *nvox, int32_t *kdim);
int epgx_coords_upload(struct epgx_coords *c, const double *k, const int32_t *nlive, int64_t nsrc);
int epgx_coords_download(const struct epgx_coords *c, double *k, int32_t *nlive);
int epgx_coords_widen(struct epgx_coords *dst, const struct epgx_coords *src);

/* epgx_state_prune_shift: (dst, cdst) = the shift of (src, csrc), per voxel v by
 *   s(v) = table[sum_d i_d(v) * sstride[d]][kdim],  i_d(v) the index of v along axis d of the C-ordered grid shape[ndim]
 * (an axis the shift does not vary along has sstride 0; table is host [ntable][kdim], already multiplied by ktvalue).
 * Wavenumbers are coordinates * ktvalue[c] on the way in and divided by it on the way out.  Per voxel: Z of row i stays at
 * k_i, F goes to k_i + s, column 1 mirrors it; cells are rnd(k / grid[c]) with rnd(x) = trunc(x - 0.5 + (x > 0)); candidates
 * that share a cell merge (sums in ascending row from +0; merged coordinate sum w k / (sum w + (sum w < 1e-12)), w the modulus
 * of the source in this voxel); with nmax >= 0 and more than nmax positive rows the centre row and the nmax rows of largest
 * sum_c |.|^2 stay; with prune != 0 the rows with sqrt(sum_c |.|^2) <= tol leave (never the centre row).  The live rows are
 * stored in lexicographic order of their cells.  *max_live = the largest live count of a voxel.  dst takes the densities of
 * src.  Deterministic, no atomics: a voxel's bits depend on the voxel alone.  The call synchronises the context's stream.
 * Errors (nothing is launched): EPGX_ERR_INVALID for a NULL argument, objects of another context, dst == src, different
 * nvox or kdim, ndim outside 1 .. 8, a grid that does not hold nvox voxels, a table index outside the table, a non-positive
 * grid, a zero ktvalue, a value that is not finite; EPGX_ERR_UNSUPPORTED for states of another capacity than 64.
 * After the launch: EPGX_ERR_UNSUPPORTED if some voxel keeps more than 64 stored orders after trim and prune; src and csrc
 * are untouched, dst and cdst are to be dropped. */
int epgx_state_prune_shift(epgx_ctx *ctx, epgx_state *dst, struct epgx_coords *cdst, const epgx_state *src, const struct epgx_coords *csrc,
                           const double *table, int64_t ntable, int32_t ndim, const int64_t *shape, const int64_t *sstride,
                           const double *ktvalue /*[kdim]*/, const double *grid /*[kdim]*/, int32_t nmax, int32_t prune, double tol,
                           int32_t *max_live);

/* epgx_state_prune_read: F0 with a time coordinate (kdim 4; statematrix.py:149-155) and per-voxel coordinates,
 *   out[v] = sum over the rows of v whose three wavenumber coordinates are within 1e-8 of zero of F exp(-|t tvalue|),
 * out: DEVICE complex128 [nvox], 16-byte aligned.  Stream-ordered, not synchronised. */
int epgx_state_prune_read(epgx_ctx *ctx, const epgx_state *st, const struct epgx_coords *c, double tvalue, void *out);

/* ---- run ------------------------------------------------------------------------------ */
/* Apply operators [op_begin, op_end) of `plan` to voxels [vox0, vox0+nvox) of the plan's grid.
 *   in  : state to start from (its voxel j is grid voxel vox0+j), or NULL = equilibrium
 *   out : where the final state goes (may be `in` for in-place), or NULL = discard
 *   signal : device pointer, complex128 [n_adc][signal_ld]; voxel vox0+j writes column
 *            signal_col0 + j; NULL if the range holds no ADC
 *   K   : k-state capacity when both in and out are NULL (else taken from the states):
 *         64 .. 1024; 2048 (four wavefronts per voxel; T / T0 / E operators, shifts by +-1, probes, SPOILER / RESET / PD);
 *         plans with derivative states: up to 1024, at 1024 with ONE variable per plan (EPGX_ERR_UNSUPPORTED otherwise);
 *         or 16 / 32 for short state matrices (state-resident only; shifts by +-1,
 *         T / T0 / E operators and probes, at K = 16 also EPGX_OP_GS / EPGX_OP_D whose tables are then
 *         laid out [3][16] -- EPGX_ERR_UNSUPPORTED otherwise).  Longer state matrices: epgx_run_tiled
 * With in = out = NULL the state never leaves registers (state-resident mode); calling it once
 * per echo with in = out streams the state through HBM once per call (per-timestep mode).
 * State-resident launches from equilibrium at K >= 256 whose records mostly run while the state matrix is still short (every
 * shift adds one order: epgpy/shift.py:86,98) walk them with 1, 2, 4 .. K / 64 orders per lane -- the same bits
 * (run_contig_grow_kernel).  At K = 128 the same kernel takes the launch, in place of the four-voxels-per-wavefront kernel
 * below, when at least 60 % of the records run while at most 64 orders can hold anything (with EPGX_CGROW=2 in the
 * environment: whenever the larger capacities would take it) -- again the same bits.
 * One wavefront owns one voxel for the whole range, except in state-resident launches with
 * K <= 128 of ranges made of T / T0 / E / S(+-1) / probe operators only: there one wavefront owns
 * four voxels (16 lanes each, K / 16 orders per lane) -- same results, bit for bit; except rotations about x
 * at K = 64, which that kernel evaluates in a sum / difference form (16 instead of 18 instructions per order
 * slot): the same products in another association order, i.e. the last bits may differ (<= 1e-13 on O(1)
 * signals) from a per-timestep run of the same plan. */
int epgx_run(epgx_ctx *ctx, const epgx_plan *plan, int32_t op_begin, int32_t op_end,
             int64_t vox0, int64_t nvox, const epgx_state *in, epgx_state *out, int32_t K,
             void *signal, int64_t signal_ld, int64_t signal_col0);

/* Which kernel epgx_run would launch for operators [op_begin, op_end) at capacity K with these states (the same checks and the
 * same decision, no launch): its name with template arguments, e.g. "rows_grow_kernel<1>", "run_kernel<1, 2, true>",
 * "drun_kernel<1, 2, 309, 0>".  The decision depends on the plan, the range, K and whether states are given -- never on the
 * number of voxels.  For tests and tools that pin the kernel of a configuration. */
int epgx_kernel_for(epgx_ctx *ctx, const epgx_plan *plan, int32_t op_begin, int32_t op_end, int32_t K, const epgx_state *in,
                    epgx_state *out, char *name_out, int64_t name_bytes);

/* The whole plan over voxels [vox0, vox0 + nvox) for state matrices of ANY length (the reference's unbounded growth,
 * epgpy/shift.py:86,98): the state lives in HBM as two buffers [nvox][3][Kbuf] c128 that alternate, cut into tiles of W
 * orders; one wavefront owns one (voxel, tile) and runs a BLOCK of records in registers on a window of the tile plus H orders
 * on either side (every shift by one spoils one order at each edge of the window, so the tile is exact after a block whose
 * shifts add up to at most H).  Only the tiles that can hold anything after a block are launched.  A record that shifts by
 * more than H orders is a launch of its own (a copy with the k = 0 fold).  The library cuts the plan into blocks.
 *   in     : start state (any epgx_state, K <= 1024, nvox voxels) or NULL = equilibrium; it is not modified
 *   Kbuf   : a multiple of 64, at least the highest order the plan can populate + 1 (counted from in->K - 1 with a start state)
 *   signal : as for epgx_run (column signal_col0 + j)
 *   slab_voxels : voxels per slab (0: the library's choice -- two buffers of at most 8 GiB; EPGX_SLAB_VOXELS lowers it)
 * Plans: T / T0 / MAT / MAT0 / E / S (any integer shift) / probes / SPOILER / RESET / PD; one GPU.
 * Errors: EPGX_ERR_INVALID (arguments, Kbuf too small or not a multiple of 64, in->K > Kbuf), EPGX_ERR_UNSUPPORTED
 * (derivative states, EPGX_OP_X / EPGX_OP_GS / EPGX_OP_D in the plan, in->K > 1024), EPGX_ERR_NOMEM (the buffers of one slab), EPGX_ERR_HIP. */
int epgx_run_tiled(epgx_ctx *ctx, const epgx_plan *plan, int64_t vox0, int64_t nvox, const epgx_state *in, int32_t Kbuf,
                   void *signal, int64_t signal_ld, int64_t signal_col0, int64_t slab_voxels);

/* The schedule epgx_run_tiled would follow for `plan` at Kbuf (no launch): blocks = launches of the tiled kernel, shifts =
 * launches of the copy kernel for shifts by more than H orders, tile_launches = sum over all launches of the tiles covered,
 * peak = the highest order that can hold anything, names = the kernel names separated by " + ", e.g.
 * "tiled_kernel<8, 32> + tiled_shift".  top0: highest order of the start state (0 from equilibrium).  Any output may be NULL. */
int epgx_tiled_info(epgx_ctx *ctx, const epgx_plan *plan, int32_t Kbuf, int32_t top0, int32_t *blocks, int32_t *shifts,
                    int64_t *tile_launches, int32_t *peak, char *names, int64_t name_bytes);

/* epgx_run_tiled for a FIRST-ORDER DERIVATIVE plan (n_vars = 1 or 2): Jacobians of state matrices of any length.  The state
 * and its n_vars derivative states live in HBM as two alternating buffers [nvox][1 + n_vars][3][Kbuf] c128 (the derivative
 * states start at zero; a start state carries no partials); one wavefront keeps the 1 + n_vars windows of its (voxel, tile)
 * in registers (tiled_deriv_kernel<8, 32, NSP, n_vars>) and walks the block with the record semantics of epgx_run's
 * derivative kernels: derivative states carry no equilibrium term, SPOILER acts on them only under
 * EPGX_DERIV_THROUGH_PLAIN_OPS, RESET and PD-with-reset always clear them.  Blocks, halos and tiles are those of
 * epgx_run_tiled.  Arguments as for epgx_run_tiled; the signal takes 1 + n_vars rows per ADC (the layout epgx_run writes for a
 * derivative plan).  Slabs: 8 GiB for the two buffers, (1 + n_vars) times the bytes per voxel.
 * Errors as for epgx_run_tiled; EPGX_ERR_UNSUPPORTED also for n_vars = 0 or > 2 and for second-order plans (EPGX_DERIV_SECOND). */
int epgx_run_tiled_deriv(epgx_ctx *ctx, const epgx_plan *plan, int64_t vox0, int64_t nvox, const epgx_state *in, int32_t Kbuf,
                         void *signal, int64_t signal_ld, int64_t signal_col0, int64_t slab_voxels);

/* epgx_tiled_info for epgx_run_tiled_deriv: the same schedule, names e.g. "tiled_deriv_kernel<8, 32, 1> + tiled_shift" (orders
 * per lane, halo, derivative states per launch). */
int epgx_tiled_deriv_info(epgx_ctx *ctx, const epgx_plan *plan, int32_t Kbuf, int32_t top0, int32_t *blocks, int32_t *shifts,
                          int64_t *tile_launches, int32_t *peak, char *names, int64_t name_bytes);

/* The whole plan, state-resident, over voxels [vox0, vox0 + nvox) in SLABS whose signal columns travel to the host while
 * the next slab computes (second stream + events): what a caller with host buffers waits for is then the PCIe copy
 * alone.
 *   signal_dev : device scratch [n_adc][dev_ld] c128, voxel vox0 + j in column j
 *   signal_host: [n_adc][host_ld] c128, voxel vox0 + j lands in column host_col0 + j.  Page-locked memory
 *                (epgx_host_alloc) receives the copies directly; ORDINARY (pageable) memory -- e.g. a fresh NumPy array
 *                of a caller that keeps every result, or a 16 GB result no pool should pin -- is filled through the
 *                context's ring of page-locked staging blocks by host threads that copy block k into place while
 *                block k + 1 crosses PCIe (HIP's own pageable path reaches 17 GB/s, this one the link rate)
 *   slab       : voxels per launch (0: chosen by the library)
 * Several contexts (GPUs) may run their ranges of one grid into one host array concurrently, each from its own host
 * thread (epgpy_amd `simulate(..., ngpu=N)`).  Synchronises the context before returning.
 *   host_dtype : enum epgx_signal_dtype of `signal_host` (host_ld / host_col0 count records of that type).  EPGX_SIGNAL_C64:
 *                every slab is narrowed on the device (epgx_signal_narrow into scratch of the context) before it leaves */
int epgx_run_to_host(epgx_ctx *ctx, const epgx_plan *plan, int32_t K, int64_t vox0, int64_t nvox, void *signal_dev,
                     int64_t dev_ld, void *signal_host, int64_t host_ld, int64_t host_col0, int64_t slab, int32_t host_dtype);
/* complex128 records src[rows][src_ld] (the first `cols` of every row) -> complex64 dst[rows][dst_ld], on the device, in the
 * context's stream order.  For consumers that move records themselves (epgx_download_2d, epgx_comm_gather) at half the bytes. */
int epgx_signal_narrow(epgx_ctx *ctx, const void *src, int64_t src_ld, void *dst, int64_t dst_ld, int64_t rows, int64_t cols);
/* The copy half alone: rows x width_bytes from device memory (row pitch dev_pitch bytes) into host memory (row pitch
 * host_pitch), through the same pipeline -- direct when `host` is page-locked, staged + host threads otherwise.  Ordered
 * behind the work already enqueued on the context's stream; synchronises before returning. */
int epgx_download_2d(epgx_ctx *ctx, void *host, int64_t host_pitch, const void *dptr, int64_t dev_pitch,
                     int64_t width_bytes, int64_t rows);

/* Weighted reduction of signal rows over grid axes, on the device: what Adc(weights=..., reduce=...)
 * computes on the host in the reference (epgpy/probe.py:141-165: arr * weights, then arr.sum(axis)).
 *   out[r][o] = sum_j  w(o, j) * signal[row0 + r * row_step][voxel(o, j)],     r = 0 .. n_rows-1
 * o runs over the kept axes of the grid, j over the axes with reduce_axis[d] != 0 (both C order).
 * weights: device pointer to complex128 values addressed with weight_strides[d] (in elements, 0 on
 * axes the weights do not depend on), or NULL for a plain sum.  out: device, [n_rows][n_out] c128.
 * The buffer may hold a voxel SLAB of the grid only (multi-GPU runs: every rank reduces what it simulated, the partial
 * sums then meet in epgx_comm_reduce): column j of `signal` is grid voxel vox0 + j, j < nvox; voxels outside the slab
 * count as zero.  vox0 = 0, nvox = the whole grid: the plain case. */
int epgx_signal_reduce(epgx_ctx *ctx, const void *signal, int64_t signal_ld, int32_t row0,
                       int32_t row_step, int32_t n_rows, int32_t ndim, const int64_t *grid_shape,
                       const uint8_t *reduce_axis, const void *weights, const int64_t *weight_strides,
                       void *out, int64_t vox0, int64_t nvox);

/* Cramer-Rao lower bounds from a Jacobian that stays on the device: what stats.crlb / stats.crlb_split compute on a downloaded
 * array in the reference (epgpy/stats.py:6-54), per voxel v = vox0 .. vox0 + nvox - 1,
 *   I(v) = 1 / sigma2 * Re( J(v)^H J(v) ),   lb(v) = I(v)^-1,
 *   out[v - vox0]             = sum_p W_p lb_pp(v)                  (flags without EPGX_CRLB_SPLIT)
 *   out[p * nvox + v - vox0]  = W_p lb_pp(v),  p = 0 .. nparam - 1    (EPGX_CRLB_SPLIT)
 * and log10 of these with EPGX_CRLB_LOG10.  J(v) is [nrec][nparam]: entry (r, c) is the complex128 value
 *   signal[r * record_stride + rows[c] * row_stride + v]
 * (strides in elements of 16 bytes) -- the layout of a Jacobian probe's records, [record][probe][row][voxel]: record_stride =
 * nprobe * nrow * nvox of the grid, row_stride = nvox of the grid, `signal` at row 0 of the probe in record 0.
 *   nrow    : rows of one probe in a record (bounds rows[c]); record_stride >= nrow * row_stride
 *   rows    : host [nparam], the row of every column, 0 .. nrow - 1, in any order, any subset; nparam = 1 .. 4
 *   weights : host [nparam] or NULL (= 1);  sigma2 > 0
 *   flags   : EPGX_CRLB_SPLIT | EPGX_CRLB_LOG10
 *   out     : DEVICE, float64 [nvox], with EPGX_CRLB_SPLIT [nparam][nvox]
 * A voxel whose information matrix is singular -- a Cholesky pivot <= 0 or not finite -- gets NaN in every output (the
 * reference: cond(I) > 1e30); never an error.  The bits of a voxel's result depend on its own records, nrec and the
 * arguments, not on nvox, vox0 or other voxels (csrc/epgx_stats.hip).  Stream-ordered; nothing is uploaded or synchronised.
 * Errors (nothing is launched): EPGX_ERR_INVALID for a NULL or misaligned pointer, nparam outside [1, 4], nrec < 1, nrow < 1,
 * a row outside [0, nrow), strides whose extent (nrec - 1) * record_stride + nrow * row_stride overflows or that overlap (row_stride < vox0 + nvox, record_stride < nrow * row_stride), vox0 < 0,
 * nvox < 0, sigma2 that is not a positive finite number, a weight that is not finite, unknown flags.  nvox = 0: nothing to do. */
enum epgx_crlb_flags { EPGX_CRLB_SPLIT = 1, EPGX_CRLB_LOG10 = 2 };
int epgx_signal_crlb(epgx_ctx *ctx, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec,
                     int32_t nparam, const int32_t *rows, int64_t vox0, int64_t nvox, const double *weights, double sigma2,
                     int32_t flags, void *out);

/* The cost of epgx_signal_crlb (without EPGX_CRLB_SPLIT) and its gradient with respect to nx design variables, from second
 * derivatives that stay on the device as well (epgpy/stats.py:31-33, stats.crlb(J, H) of the reference), per voxel v:
 *   S = lb diag(W) lb,   G_x[a][b] = sum_r Re( conj(H_rax) J_rb ),
 *   out_cost[v - vox0]             = sum_p W_p lb_pp(v)                        -- the bits epgx_signal_crlb writes
 *   out_grad[x * nvox + v - vox0]  = -2 / sigma2 * sum_ab S_ab G_x[a][b],     x = 0 .. nx - 1
 * and with EPGX_CRLB_LOG10 log10(cost) and grad / (cost ln 10).  The Jacobian (signal ... nvox) as for epgx_signal_crlb.
 * H_rax, the derivative of column a of the Jacobian with respect to design variable x in record r, is the complex128 value
 *   hess[offsets[a * nx + x] + r * record_strides[a * nx + x] + v]
 * (elements of 16 bytes): the layout of a DeviceHessian, whose entries lie in the passes of their variable pairs.
 *   hess, hess_len   : DEVICE buffer and its length in elements
 *   offsets, record_strides : host [nparam][nx]; offsets < 0: the entry is identically zero and nothing is read for it
 *   weights, sigma2  : as for epgx_signal_crlb;  flags: EPGX_CRLB_LOG10 only
 *   out_cost         : DEVICE, float64 [nvox];  out_grad: DEVICE, float64 [nx][nvox]
 * A singular voxel (epgx_signal_crlb) gets NaN in the cost and in all nx gradient entries.  A voxel's bits depend on its own
 * records, nrec and the arguments only.  One launch per 4 design variables, stream-ordered; nothing is uploaded or synchronised.
 * Errors (nothing is launched): EPGX_ERR_INVALID for what epgx_signal_crlb refuses, EPGX_CRLB_SPLIT, nx < 1, and any entry with
 * offset >= 0 whose last record ends outside the buffer (offset + (nrec - 1) * stride + vox0 + nvox > hess_len) or whose records
 * overlap (nrec > 1 and stride < nvox). */
int epgx_signal_crlb_grad(epgx_ctx *ctx, const void *signal, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec,
                          int32_t nparam, const int32_t *rows, int64_t vox0, int64_t nvox, const void *hess, int64_t hess_len,
                          int32_t nx, const int64_t *offsets, const int64_t *record_strides, const double *weights, double sigma2,
                          int32_t flags, void *out_cost, void *out_grad);

/* Dictionary matching on records that stay on the device (csrc/epgx_match.hip): the consumer of a dictionary left in HBM by
 * simulate(..., out="device").  Dictionary D[t][a] = dict[t * dict_row_stride + a], records t = 0 .. nrec - 1, atoms a = 0 ..
 * natoms - 1; measured signals S[t][m] = sig[t * sig_row_stride + m], m = 0 .. nmeas - 1; complex128, strides in elements of 16
 * bytes.
 *   n_a      = sum_t |D[t,a]|^2                                        (epgx_signal_norms: out[a], once per dictionary)
 *   c[a,m]   = sum_t conj(D[t,a]) S[t,m],     q[a,m] = |c[a,m]|^2 / n_a
 *   out_index[m] = argmax_a q[a,m] over the atoms whose n_a is a finite number > 0; among equal q the LOWEST a
 *   out_scale[m] = c[idx,m] / n_idx             (the complex proton density: S[:,m] ~ scale D[:,idx])
 *   out_score[m] = sqrt(q[idx,m] / sum_t |S[t,m]|^2), at most 1;  0 where the signal is identically zero
 * Invalid atoms: an all-zero atom or one holding a NaN / Inf is never chosen.  Where no atom is valid, or the best q is not
 * finite, the voxel gets index -1, scale 0, score 0; never an error.  (q is evaluated as (Re c^2 + Im c^2) * (1 / n_a).)
 * Invariance: the records are consumed in steps of 4 from t = 0, the tail padded with zeros, so the bits of c[a,m] depend on
 * column a, column m and nrec alone, and with them index, scale and score of a voxel -- not on nmeas, the voxel's place in
 * the call, nsplit, or other atoms and voxels.
 *   norms  : DEVICE float64 [natoms], what epgx_signal_norms wrote for this dictionary
 *   nsplit : the atoms are cut into nsplit ranges that run side by side (a small nmeas still fills the device); range s holds
 *            atoms [s * (natoms / nsplit) + min(s, natoms % nsplit), ... of the next s).  0: the library chooses.  Every (range,
 *            voxel) leaves 32 bytes in scratch of the context; a second kernel reduces the ranges by the rule above.
 *   out_index : DEVICE int64 [nmeas];  out_scale : DEVICE complex128 [nmeas];  out_score : DEVICE float64 [nmeas]
 * Both calls are stream-ordered; nothing is uploaded or synchronised.
 * Errors (nothing is launched): EPGX_ERR_INVALID for a NULL or misaligned pointer (16 bytes: dict, sig, out_scale; 8: the
 * others), nrec < 1, natoms < 1, nmeas < 0, nsplit < 0 or > natoms, dict_row_stride (row_stride) < natoms, sig_row_stride <
 * nmeas, an extent (nrec - 1) * stride + columns or a launch nsplit * ceil(nmeas / 64) that overflows.  nmeas = 0: nothing to do. */
int epgx_signal_norms(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, void *out);
int epgx_signal_match(epgx_ctx *ctx, const void *dict, int64_t dict_row_stride, const void *norms, int64_t natoms,
                      const void *sig, int64_t sig_row_stride, int32_t nrec, int64_t nmeas, int32_t nsplit,
                      void *out_index, void *out_scale, void *out_score);

/* SVD compression of a dictionary that stays on the device (csrc/epgx_compress.hip).  The caller takes the eigenvectors of the
 * Gram matrix on the host (nrec is small) and projects dictionary and measured signals onto the leading `rank` of them; matching
 * then runs on the projected records with nrec = rank.  Layouts and strides as above.
 *   G[s,t]   = sum over the atoms a whose norms[a] is a finite number > 0 of D[s,a] conj(D[t,a])       (epgx_signal_gram)
 *   out[r,c] = sum_t conj(B[t,r]) X[t,c],   B[t][r] = basis[t * rank + r],  r < rank <= 64              (epgx_signal_project)
 * epgx_signal_gram: out is DEVICE complex128 [nrec][nrec].  out[t][s] holds the exact conjugate bits of out[s][t] and the
 *   diagonal an imaginary part of exactly 0.  Invalid atoms (all zero, or holding a NaN / Inf) are replaced by zeros when they
 *   are loaded, so G is finite whatever they hold.  The atoms are cut into nsplit ranges by the rule of epgx_signal_match; every
 *   range leaves one partial Gram matrix (16 nrec^2 bytes) in scratch of the context and a second kernel adds them in ascending
 *   order.  No atomics: the bits of G depend on the valid columns of D, nrec, natoms and nsplit only.
 *   nsplit = 0: the library takes  min(ceil(2048 / npair), max(natoms / 1024, 1)),  npair = nblock (nblock + 1) / 2,
 *   nblock = ceil(nrec / 64)  -- a function of (nrec, natoms) alone, not of the device or the pool, so that the same dictionary
 *   gives the same G on every machine.
 * epgx_signal_project: basis is DEVICE complex128 [nrec][rank]; src [nrec] rows of src_row_stride, out [rank] rows of
 *   out_row_stride elements, ncol columns each.  Every column of src is read once whatever the rank.  The records are consumed in
 *   steps of 4 from t = 0, the tail padded with zeros: the bits of out[r,c] depend on column c of src, column r of basis and nrec
 *   alone -- not on ncol, rank, the column's place in the call or the strides.  Non-finite values propagate to their column.
 * Both calls are stream-ordered; nothing is uploaded or synchronised.
 * Errors (nothing is launched or written): EPGX_ERR_INVALID for a NULL or misaligned pointer (16 bytes; norms 8), nrec < 1,
 * natoms < 1, ncol < 0, nsplit < 0 or > natoms, rank < 1, > 64 or > nrec, dict_row_stride < natoms, src_row_stride or
 * out_row_stride < ncol, an extent (rows - 1) * stride + columns, a scratch size or a launch that overflows.  ncol = 0: nothing
 * to do. */
int epgx_signal_gram(epgx_ctx *ctx, const void *dict, int64_t dict_row_stride, const void *norms, int32_t nrec, int64_t natoms,
                     int32_t nsplit, void *out);
int epgx_signal_project(epgx_ctx *ctx, const void *basis, int32_t rank, const void *src, int64_t src_row_stride, int32_t nrec,
                        int64_t ncol, void *out, int64_t out_row_stride);

/* Single-precision matching (csrc/epgx_match32.hip): the calls above on complex64 records, elements of 8 bytes (float re, im),
 * pointers aligned to 8 bytes, strides in elements of 8 bytes.  A complex64 dictionary is DEFINED as the complex128 one rounded
 * once, per component, to nearest even, subnormals kept, overflow to +-Inf (NumPy's astype(complex64)), and matching on the
 * rounded operands D32, S32 as
 *   n_a      = sum_t |D32[t,a]|^2, accumulated in fp64 in record order           (epgx_signal_norms_c64: out[a] float64)
 *   c[a,m]   = sum_t conj(D32[t,a]) S32[t,m], accumulated in fp32 (v_mfma_f32_16x16x4_f32: an exact k-ordered fmaf chain)
 *   q[a,m]   = (Re c^2 + Im c^2) * (1 / n_a), evaluated in fp64 from the fp32 c
 * with the rule, the invalid atoms, out_index / out_scale / out_score (int64, complex128, float64; scale = c / n and score =
 * sqrt(q / sum_t |S32[t,m]|^2) in fp64), nsplit and the scratch of epgx_signal_match.  The records of a pair are consumed in
 * steps of 4 from t = 0, the tail padded with zeros: the bits of c[a,m] depend on column a, column m and nrec alone.
 * The rounding itself is epgx_signal_narrow above (rows of any stride on both sides; the source is only read).
 * Both calls are stream-ordered; nothing is uploaded or synchronised.
 * Errors (nothing is launched): EPGX_ERR_INVALID for a NULL or misaligned pointer (16 bytes: out_scale; 8: the others),
 * nrec < 1, natoms < 1, nmeas < 0, nsplit < 0 or > natoms, dict_row_stride (row_stride) < natoms, sig_row_stride < nmeas, an
 * extent (nrec - 1) * stride + columns or a launch nsplit * ceil(nmeas / 64) that overflows.  nmeas = 0: nothing to do. */
int epgx_signal_norms_c64(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int64_t natoms, void *out);
int epgx_signal_match_c64(epgx_ctx *ctx, const void *dict, int64_t dict_row_stride, const void *norms, int64_t natoms,
                          const void *sig, int64_t sig_row_stride, int32_t nrec, int64_t nmeas, int32_t nsplit,
                          void *out_index, void *out_scale, void *out_score);

/* One variable-projection Gauss-Newton step off the grid (csrc/epgx_refine.hip; within ABI 11): the consumer of the derivative
 * rows of a Jacobian left in HBM by simulate(..., probe=Jacobian, out="device").  For measured voxel m with atom a = index[m]:
 *   d_t = D[t,a] = jac[t * record_stride + a],   j_pt = J_p[t,a] = jac[t * record_stride + rows[p] * row_stride + a],  p < P = nparam,
 *   s_t = S[t,m] = sig[t * sig_row_stride + m],  all complex128, strides in elements of 16 bytes.
 * Accumulated over the records:
 *   n = sum |d|^2 (real)    E = sum |s|^2 (real)    c = sum conj(d) s    b_p = sum conj(j_p) s    h_p = sum conj(d) j_p
 *   M_pq = sum conj(j_p) j_q   (Hermitian, M_pp real; only Re M_pq enters below and only that is accumulated)
 * From those, per voxel and in float64:
 *   rho   = c / n                                       (match's scale, recomputed here from the same records)
 *   N_pq  = |rho|^2 Re(M_pq - conj(h_p) h_q / n)         Gauss-Newton matrix of  min over real delta of ||s - rho (d + J delta)||^2,
 *   y_p   = Re(conj(rho) (b_p - rho conj(h_p)))         rho projected out (Kaufman's variable projection)
 *   Nhat_pq = N_pq / (|rho|^2 sqrt(M_pp M_qq))           equilibrated by the UNPROJECTED column norms: pivots in [0, 1]
 *   delta = solution of N delta = y by Cholesky of Nhat
 *   delta_p clipped to +-limit_p where a limit is given
 *   num   = c + sum_p delta_p b_p
 *   den   = n + 2 sum_p delta_p Re h_p + sum_pq delta_p delta_q Re M_pq
 *   scale' = num / den
 *   score' = |num| / sqrt(den E)                        of the LINEARISED atom d + J delta (0 where E = 0)
 * (Nhat is evaluated as Re(M_pq - conj(h_p) h_q / n) / sqrt(M_pp M_qq); where |rho|^2 is zero or not finite -- an all-zero
 * signal -- the quotient above is 0 / 0 and every pivot counts as not finite.)
 * A voxel is UNRESOLVED where index[m] lies outside [0, natoms) (-1 included), where n or an M_pp is zero or not finite, or where a
 * Cholesky pivot of Nhat (the diagonal entry before its root) is <= rcond or not finite.  It gets NaN in every delta_p, scale' =
 * rho and score' = the unrefined score |c| / sqrt(n E) (0 where E = 0); where the index is invalid scale 0 and score 0.  Never an
 * error.  The kernel never reads an atom outside [0, natoms); a voxel with an invalid index loads nothing.
 * rcond: a pivot of 1e-10 means a Jacobian column lies within 1e-5 rad of the span of d and the earlier columns.
 * Invariance: the records are cut into 1 (nrec <= 16), 2 (<= 32), 4 (<= 64) or 8 slices by nrec alone and the slices are added
 * in ascending order, so the bits of a voxel's result depend on its own column of S, its atom's columns, nrec and the arguments
 * -- not on nmeas, the voxel's place in the call, or other voxels.
 *   jac       : DEVICE, at row 0 (the probed state) of record 0 of the probe: [record][row][atom], record_stride >= nrow * row_stride,
 *               row_stride >= natoms (the layout and stride checks of epgx_signal_crlb)
 *   rows      : host [nparam], the row of every chosen column, 1 .. nrow - 1, each once, in any order; nparam = 1 .. 4
 *   index     : DEVICE int64 [nmeas]
 *   limit     : host [nparam] of positive numbers (+Inf allowed), or NULL for no clipping;  rcond in [0, 1)
 *   out_delta : DEVICE float64 [nparam][nmeas];  out_scale : DEVICE complex128 [nmeas];  out_score : DEVICE float64 [nmeas]
 * Stream-ordered; nothing is uploaded or synchronised.
 * Errors (nothing is launched): EPGX_ERR_INVALID for a NULL (limit apart) or misaligned pointer (16 bytes: jac, sig, out_scale; 8:
 * the others), nparam outside [1, 4], nrec < 1, nrow < 1, natoms < 1, nmeas < 0, row_stride < natoms, record_stride < nrow *
 * row_stride, sig_row_stride < nmeas, an extent that overflows, rows[c] < 1 (row 0 is the state) or >= nrow, a repeated row, a
 * limit that is not positive, rcond outside [0, 1).  nmeas = 0: nothing to do. */
int epgx_signal_refine(epgx_ctx *ctx, const void *jac, int64_t record_stride, int64_t row_stride, int32_t nrow, int32_t nrec,
                       int32_t nparam, const int32_t *rows, int64_t natoms, const void *sig, int64_t sig_row_stride, int64_t nmeas,
                       const void *index, const double *limit, double rcond, void *out_delta, void *out_scale, void *out_score);

/* Non-negative mixtures along one grid axis of a dictionary left in HBM (csrc/epgx_nnls.hip; within ABI 11): multi-component
 * analysis (T2 spectra, myelin water fraction, partial volume).  The dictionary is read as D[t,a,g]: atom a < ncomp of the
 * component axis, group g = o * ninner + i (o < nouter, i < ninner: every other grid axis, flattened in C order), record t at
 *   dict[t * row_stride + (o * ncomp + a) * axis_stride + i]      complex128, strides in elements of 16 bytes;
 * for a C-ordered grid axis_stride = ninner = the product of the axes behind the component axis, nouter that of the axes before.
 * S[t,m] = sig[t * sig_row_stride + m].  For every voxel m and group g:
 *   H_g[a,b] = Re sum_t conj(D[t,a,g]) D[t,b,g]          (epgx_signal_component_gram: once per dictionary)
 *   f[a]     = Re sum_t conj(D[t,a,g]) S[t,m]            E = sum_t |S[t,m]|^2
 *   mu_g     = reg * (trace(H_g over the valid atoms) / (number of valid atoms))
 *   x*       = argmin over x >= 0 of  x^T (H_g + mu_g I) x - 2 f^T x + E
 * An atom is VALID where H_g[a,a] is finite and > 0 (bit a of the group's mask); an invalid atom gets weight 0 and is never a candidate.
 * Method: Lawson and Hanson's active set on the Gram form.  From x = 0 and an empty passive set P, the atom outside P with the
 * largest w_a = f_a - ((H_g + mu_g I) x)_a enters, the LOWEST a among equal w, while w_a > tol sqrt(H_g[a,a] E); P is solved by
 * Cholesky of (H_g + mu_g I)[P,P] in the order the atoms entered; while a solution s has an entry <= 0 the iterate moves by
 * alpha = min x_p / (x_p - s_p) over those entries towards s, and they leave where they reach 0 or set alpha.  In the end
 * J = E - sum_a x_a (f_a + w_a).
 * Per voxel: the weights of the chosen group; the group (group = NULL: the g of the smallest finite J, the LOWEST g among equal J;
 * else group[m]); residual = sqrt(max(J - mu_g |x|^2, 0)); status 0: solved, 1: the cap of 3 ncomp passive-set solves was reached
 * (the weights are the last feasible iterate), 2: a pivot was not finite or <= 0, or E, an f_a, an entry of a solution or J was
 * not finite (such a group is skipped).  Where every group is skipped, or group[m] lies outside [0, G): group -1, NaN weights,
 * NaN residual, status 2; a voxel with such a group[m] reads nothing.  An all-zero signal: weights 0, status 0, residual 0, in
 * group 0 of the search.  Never an error.
 * Invariance: every sum runs in a fixed order (records, passive positions and atoms ascending) and the groups are compared in
 * ascending order inside the wavefront that owns the voxel, so the bits of a voxel's result depend on its own column of S, the
 * dictionary and the arguments -- not on nmeas, the voxel's place in the call, or other voxels.  H_g is symmetric to the bit.
 *   out_gram  : DEVICE float64 [G][ncomp][ncomp];  out_mask : DEVICE uint64 [G]            (G = nouter * ninner)
 *   gram, mask: DEVICE, what epgx_signal_component_gram wrote for the same dictionary and decomposition
 *   group     : DEVICE int64 [nmeas], or NULL
 *   out_weights : DEVICE float64 [ncomp][nmeas];  out_group : DEVICE int64 [nmeas];  out_residual : DEVICE float64 [nmeas];
 *   out_status  : DEVICE int32 [nmeas]
 * Stream-ordered; nothing is uploaded or synchronised.
 * Errors (nothing is launched): EPGX_ERR_INVALID for a NULL (group apart) or misaligned pointer (16 bytes: dict, sig; 4: out_status;
 * 8: the others), ncomp outside [1, 64], nrec < 1, nouter < 1, ninner < 1, axis_stride < ninner, more than 2^31 - 1 groups or
 * voxels, a row_stride that does not hold the atoms, sig_row_stride < nmeas, an extent that overflows, nmeas < 0, reg or tol
 * negative or not finite.  nmeas = 0: nothing to do. */
int epgx_signal_component_gram(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride,
                               int64_t nouter, int64_t ninner, void *out_gram, void *out_mask);
int epgx_signal_nnls(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride,
                     int64_t nouter, int64_t ninner, const void *gram, const void *mask, const void *sig, int64_t sig_row_stride,
                     int64_t nmeas, double reg, double tol, const void *group, void *out_weights, void *out_group,
                     void *out_residual, void *out_status);

/* The chi^2-driven ridge of the non-negative mixtures (csrc/epgx_nnls_chi2.hip; within ABI 11): the discrepancy principle of
 * multi-component T2 analysis (Whittall and MacKay; DECAES).  Per voxel, with the notation of epgx_signal_nnls, J(x; mu) =
 * x^T (H_g + mu I) x - 2 f^T x + E at its minimiser x(mu) >= 0 and Jd(mu) = J - mu |x(mu)|^2 the data misfit:
 *   1. Group and baseline: exactly epgx_signal_nnls at mu_0 = reg * mean valid H_g[a,a] -- every group (group = NULL) or group[m],
 *      the g of the smallest finite J, the lowest among equal.  x_0 its weights, Jd_0 = Jd(mu_0).  Regularisation never changes
 *      the group.  Status 1 and 2 of this fit pass through: its weights (NaN), residual, mu = mu_0 (NaN), chi2 = 1 (NaN), evals 0.
 *   2. Status 4 where Jd_0 <= 0 or Jd_0 < 4 * 8 (nrec + ncomp) 2^-53 E / chi2_rtol, four times the rounding of the Gram-form J over
 *      chi2_rtol: the ratio cannot be resolved; x_0, mu = mu_0, chi2 = 1, evals 0.  (An all-zero signal is such a voxel.)
 *   3. Target T = chi2 * Jd_0.  |Jd_0 / T - 1| <= chi2_rtol: status 0 at mu_0, evals 0.  T >= E (x = 0 has the misfit E: no ridge
 *      reaches T): status 3 at mu_0, evals 0.
 *   4. Search, every evaluation one COLD fit (x = 0, empty passive set) at its mu, r(mu) = Jd(mu) / T - 1:
 *      bracket: mu = 16 mu_lo from mu_lo = mu_0 while r(mu) < -chi2_rtol; then Illinois regula falsi in log mu,
 *        mu = mu_lo exp(r_lo / (r_lo - r_hi) log(mu_hi / mu_lo)),
 *      the new point replaces the end of its sign, and where the same end is replaced twice running the r of the other end is
 *      halved.  |r(mu)| <= chi2_rtol ends the search: status 0, the weights at that mu.  After max_evals fits, at a fit that is not
 *      status 0 (the cap of 3 ncomp solves, a pivot) or a mu that is not finite the search ends with status 3 at the evaluated
 *      point of the largest Jd <= T, the baseline if no other.
 * Jd is non-decreasing in mu for the constrained problem, so the root is bracketed from mu_0 upward.
 * Per voxel: weights, group, residual = sqrt(max(Jd, 0)) of the returned weights, status (0, 1, 2 as above; 3, 4), out_mu the
 * ridge of the returned weights, out_chi2 = Jd / Jd_0, out_evals the fits of step 4 (the baseline is not counted).
 * Invariance as for epgx_signal_nnls: one wavefront (one block) per voxel, the sums of the fit in their fixed order, the search a
 * fixed function of the voxel's Jd values; exp and log are the device's.
 *   group     : DEVICE int64 [nmeas], or NULL: nnls_kernel runs first and its out_group is read on the device
 *   max_evals : the cap of step 4, 0 .. 40 (NNLS_CHI2_EVALS of csrc/epgx_nnls.h; smaller values are for tests)
 *   out_mu, out_chi2 : DEVICE float64 [nmeas];  out_evals : DEVICE int32 [nmeas];  the others as for epgx_signal_nnls
 * Stream-ordered; nothing is uploaded or synchronised.
 * Errors (nothing is launched): those of epgx_signal_nnls; NULL or misaligned out_mu, out_chi2 (8 bytes), out_evals (4); reg = 0
 * (the bracket grows from mu_0); chi2 not a finite number > 1; chi2_rtol outside (0, 1); max_evals outside [0, 40].  nmeas = 0:
 * nothing to do. */
int epgx_signal_nnls_chi2(epgx_ctx *ctx, const void *dict, int64_t row_stride, int32_t nrec, int32_t ncomp, int64_t axis_stride,
                          int64_t nouter, int64_t ninner, const void *gram, const void *mask, const void *sig, int64_t sig_row_stride,
                          int64_t nmeas, double reg, double tol, const void *group, double chi2, double chi2_rtol, int32_t max_evals,
                          void *out_weights, void *out_group, void *out_residual, void *out_status, void *out_mu, void *out_chi2,
                          void *out_evals);

/* Convenience for bindings that only have host arrays (what a ctypes/NumPy binding inside
 * the reference would call once per simulate()): builds the plan, runs the whole sequence
 * state-resident over the full grid, copies signal (and optionally the final state) back. */
int epgx_simulate_f64(epgx_ctx *ctx, const epgx_plan_desc *desc, int32_t K,
                      const double *init_half /*nullable [nvox][3][K]*/,
                      const double *density /*nullable [nvox]*/,
                      void *signal_out /*[n_adc][nvox] records of signal_dtype*/,
                      double *state_out /*nullable [nvox][3][K]*/,
                      int32_t signal_dtype /* enum epgx_signal_dtype */);

/* Same, with the voxel range split into contiguous slabs over the first `ngpu` devices of this process (results are
 * identical to the 1-GPU call).  The result is a HOST array, so nothing is gathered on the device side: every GPU runs
 * its slab through the epgx_run_to_host pipeline into its own columns of `signal_out` -- ngpu PCIe links in parallel,
 * no collective, no dependency on librccl.  (Device-resident consumers gather with epgx_comm_* below; with the
 * environment variable EPGX_SHARDED_GATHER=rccl this entry point also takes that route -- slabs to GPU 0 over
 * ncclSend / ncclRecv on a communicator set that is created once per process and `ngpu` -- which is how the
 * single-process form of the gather is exercised on a test box.) */
int epgx_simulate_sharded_f64(const epgx_plan_desc *desc, int32_t K, int32_t ngpu,
                              const double *density /*nullable*/, void *signal_out /*[n_adc][nvox] records of signal_dtype*/,
                              int32_t signal_dtype /* enum epgx_signal_dtype */);

/* ---- multi-GPU: the signal slabs meet ONCE, over RCCL / xGMI ---------------------------- */
/* The reference's only parallel attempt is the commented-out `simulate_parallel`
 * (epgpy/functions.py:195-248): a process pool over chunks of the parameter grid whose results are
 * concatenated at the end.  Here every rank (one process per GPU) simulates a contiguous voxel slab and
 * the slabs meet ONCE, on the device, over RCCL point-to-point transfers (ncclSend / ncclRecv in one
 * group: every peer uses its own xGMI link to the root) -- or, for probes that sum over grid axes
 * (Adc(weights=, reduce=), epgpy/probe.py:141-165), as ONE ncclReduce of the ranks' partial sums, so that
 * only the reduced records travel.  librccl.so.1 is loaded when the first of these functions is called; a
 * process that never calls them never pays for it.
 *   rank 0:      epgx_comm_unique_id(id)  -> hand the 128 bytes to every rank (any side channel)
 *   every rank:  epgx_comm_create(ctx, id, rank, world_size, &comm)      (collective; keep the communicator:
 *                creating one costs 0.1 - 1 s)
 *   every rank:  epgx_comm_gather(comm, slab, gathered, nbytes, root)    (collective)
 * `gathered` (root only; NULL elsewhere) holds world_size blocks of `nbytes`, block r = rank r's slab;
 * the root may have written its own slab straight into its block (send == gathered + rank * nbytes).
 * `nbytes` must be a multiple of 8 and the same on every rank.
 *
 * Stream order.  A communicator owns a side stream.  Every transfer below is enqueued THERE, behind an event that
 * marks what the context's stream holds at the time of the call -- so a rank can keep launching kernels for its
 * next sub-slab while the previous one is on the wire -- and epgx_comm_join makes the context's stream wait for
 * all transfers enqueued so far (no host synchronisation anywhere).  epgx_comm_gather = epgx_comm_gather_part
 * + epgx_comm_join. */
#define EPGX_COMM_ID_BYTES 128
typedef struct epgx_comm epgx_comm;
int epgx_comm_unique_id(void *id_out /* EPGX_COMM_ID_BYTES */);
int epgx_comm_create(epgx_ctx *ctx, const void *id, int32_t rank, int32_t world_size, epgx_comm **out);
int epgx_comm_destroy(epgx_comm *comm);
int epgx_comm_count(const epgx_comm *comm, int32_t *n_ranks); /* ncclCommCount: the ranks RCCL itself sees in the communicator */
int epgx_comm_gather(epgx_comm *comm, const void *send, void *gathered, int64_t nbytes, int32_t root);
/* One PART of a pipelined gather: like epgx_comm_gather, but rank r's `nbytes` land at gathered + r * block_stride
 * (block_stride >= nbytes, bytes), and the context's stream does not wait for the transfer (epgx_comm_join does).
 * A rank that cuts its slab into sub-slabs [n_adc][sub] laid out one after the other sends sub-slab k while it
 * computes sub-slab k + 1:  gathered = base + k * sub_bytes, block_stride = bytes of a whole rank block. */
int epgx_comm_gather_part(epgx_comm *comm, const void *send, void *gathered, int64_t nbytes, int64_t block_stride,
                          int32_t root);
int epgx_comm_join(epgx_comm *comm);
/* Sum of `count` doubles over all ranks, result at the root (recv: root only; may equal send): ncclReduce(ncclDouble,
 * ncclSum).  What Adc(reduce=) needs across GPUs: every rank sums over its own voxels (epgx_signal_reduce with its
 * slab), the partial sums meet here.  Enqueued like a gather part; followed by its own join. */
int epgx_comm_reduce(epgx_comm *comm, const void *send, void *recv, int64_t count, int32_t root);
/* Strided device-to-host copy of a [rows][width_bytes] block into a host array with `host_pitch` bytes
 * per row (assembles gathered slabs [n_adc][slab] into the caller's [n_adc][nvox] array during the
 * download, no host-side pass); synchronises the context's stream. */
int epgx_memcpy_d2h_2d(epgx_ctx *ctx, void *host, int64_t host_pitch, const void *dptr, int64_t dev_pitch,
                       int64_t width_bytes, int64_t rows);

#ifdef __cplusplus
}
#endif
#endif /* EPGX_H */
