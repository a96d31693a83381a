/*
 * fusionpic.h — C ABI of libfusionpic.so, the MI355X (gfx950) implementation of
 * fusion-sim's per-step particle-in-cell hot path.
 *
 * The library replaces the object returned by the reference factory
 *     empic.makeCylindricalParticlePusher(spec)          (empic.js:30-1529)
 * for the calls that sit on the hot path.  Every entry point names the
 * reference interface it stands in for (file:line under
 * /root/reference/public/javascripts/).  The JavaScript host keeps the reference's
 * method names through an N-API addon (fusion-sim_amd/js/); the binding a
 * maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes.  No C++ exception crosses the ABI.
 *   - Every call returns FPIC_OK (0) or a negative fpic_status.  The text of the
 *     last failure on a handle is fpic_last_error(h); for a failed fpic_create it
 *     is fpic_last_error(NULL).  The N-API layer turns a non-zero status into a
 *     synchronous `throw new Error(msg)`, which is how the reference reports
 *     spec and GL failures (utilities.js:118-127, :213-259).
 *   - Host buffers are caller-owned and copied during the call; no host pointer
 *     is kept.  Device buffers belong to the handle and die with fpic_destroy.
 *   - A handle is not thread-safe (the reference runs on one JS thread).
 *   - Calls enqueue on the handle's HIP stream and return; fpic_read_*,
 *     fpic_get_particles and fpic_sync wait for the stream.
 *   - There is NO CPU fallback: without a gfx950 device fpic_create fails with
 *     FPIC_ERR_NO_DEVICE.
 *
 * Grid layout at the boundary (reference: empic.js:1162, texture index
 * 4*(i + j*nr) + c with i = r index, j = z index): fpic_read_grid returns
 * exactly that RGBA float layout.  fpic_set_grid takes the reference's nested
 * JavaScript order value[i][j][k], flattened as ((i*nz + j)*ncomp + k).
 */
#ifndef FUSIONPIC_H
#define FUSIONPIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FPIC_ABI_VERSION 2

typedef enum fpic_status {
    FPIC_OK = 0,
    FPIC_ERR_INVALID_ARG = -1, /* bad spec / argument; message keeps ".prop <- ..." form */
    FPIC_ERR_NO_DEVICE = -2,   /* no gfx950 device visible: the product path has no CPU fallback */
    FPIC_ERR_HIP = -3,         /* a HIP runtime call failed */
    FPIC_ERR_OOM = -4,         /* device or host allocation failed */
    FPIC_ERR_STATE = -5        /* call made in the wrong state (e.g. step before set) */
} fpic_status;

typedef enum fpic_dtype {
    FPIC_F32 = 0,
    FPIC_F64 = 1
} fpic_dtype;

/* Grids accepted by fpic_set_grid (reference: out.set, empic.js:1157-1350). */
typedef enum fpic_grid_in {
    FPIC_GRID_E = 0,          /* [nr][nz][3]  V/m   (empic.js:1159-1177) */
    FPIC_GRID_B = 1,          /* [nr][nz][3]  T     (empic.js:1179-1197) */
    FPIC_GRID_SINK_MASK = 2,  /* [nr][nz]     alive where > 0.5 (empic.js:1246-1260) */
    FPIC_GRID_SOURCE_PDF = 3  /* [nr][nz]     un-normalised pdf -> 512x512 inverse CDF (empic.js:1263-1349) */
} fpic_grid_in;

/* Grids returned by fpic_read_grid, all RGBA, index 4*(i + j*W) + c. */
typedef enum fpic_grid_out {
    FPIC_READ_MOMENTS = 0, /* moments01      nr x nz  (empic.js:933, K4)  */
    FPIC_READ_NORM = 1,    /* moments01_norm nr x nz  (empic.js:1040, K5) */
    FPIC_READ_AVG = 2,     /* moments01_avgA nr x nz  (empic.js:1071, K6) */
    FPIC_READ_R1 = 3,      /* nr x nz, w = 1 (empic.js:506-542) */
    FPIC_READ_R2 = 4,      /* (empic.js:545-581) */
    FPIC_READ_R3 = 5,      /* (empic.js:585-621) */
    FPIC_READ_A = 6,       /* (empic.js:625-659) */
    FPIC_READ_B = 7,       /* B frame buffer incl. painters' alpha (empic.js:197) */
    FPIC_READ_E = 8,       /* (empic.js:186) */
    FPIC_READ_SINK = 9,    /* red channel only is written (empic.js:1249) */
    FPIC_READ_INV_CDF = 10 /* 512 x 512, .xy used (empic.js:228-241, :1328-1339) */
} fpic_grid_out;

/* ---- extension: spec.geometry.  The reference has ONE geometry (axisymmetric (r,z) grid, static
 * fields, empic.js:111-115) and no field solve in its step loop (empic.js:1436-1505; SURVEY.md
 * section 0).  FPIC_GEOM_CART3D is the self-consistent electrostatic mode of BASELINE.json
 * configs[2..4]: a periodic box radius x length_y x height (x, y, z) on nr x ny x nz nodes,
 * CIC gather/deposit, Poisson solve each sub-step.  It has no reference counterpart (parity
 * unpinned; defined by oracle/es3d_oracle_impl.h).  The same entry points drive it:
 *   fpic_set_particles  positions in metres (wrapped into the box), velocities in units of c
 *   fpic_add_bz / fpic_add_b   uniform external magnetic field (Boris rotation)
 *   fpic_precalc        fields <- particles: deposit + solve (the fields->coefficients stage,
 *                       empic.js:1413-1434; must precede the first step)
 *   fpic_step           2 sub-steps per call (empic.js:1436-1469), each push+deposit fused, then solve
 *   fpic_density        no-op: the charge density of the current positions is always at hand
 *   fpic_get_particles / fpic_get_cells / fpic_sort / fpic_sync / fpic_profile / fpic_get_stats
 * Calls that only make sense on the (r,z) pusher return FPIC_ERR_STATE. */
typedef enum fpic_geometry {
    FPIC_GEOM_CYL_RZ = 0, /* the reference's pusher */
    FPIC_GEOM_CART3D = 1
} fpic_geometry;

typedef enum fpic_solver {
    FPIC_SOLVER_NONE = 0,        /* fields are what fpic_set_field3 uploaded */
    FPIC_SOLVER_POISSON_FFT = 1, /* rocFFT forward/inverse around a hand-written k-space kernel */
    FPIC_SOLVER_YEE = 2          /* full EM (BASELINE configs[4]): Yee FDTD, node-centred CIC gather of E and B, charge-conserving
                                    integer current deposit (zigzag); precalc() sets E to the Poisson field of the charge on the
                                    lattice's edges and B to the uniform external field; density() deposits the charge grid */
} fpic_solver;

/* spec.shape: the deposit of density() on the (r,z) grid (SURVEY.md 8(b) key shape:'ref11'|'cic'). */
typedef enum fpic_shape {
    FPIC_SHAPE_REF11 = 0, /* the reference's 11x11 cos^2 point sprite (empic.js:949-1035) */
    FPIC_SHAPE_CIC = 1    /* extension, no reference counterpart: bilinear over the four nearest cell centres */
} fpic_shape;

/* CART3D grids, node index i + nr*(j + ny*k) (i fastest, as the reference's texel index
 * 4*(i + j*nr), empic.js:1162). */
typedef enum fpic_field3 {
    FPIC_F3_E = 0,         /* in: value[i][j][k][3] V/m;  out: 4 per node (Ex, Ey, Ez, phi) */
    FPIC_F3_RHO = 1,       /* out: C/m^3, 1 per node */
    FPIC_F3_PHI = 2,       /* out: V, 1 per node */
    FPIC_F3_RHO_FIXED = 3, /* out: int64 per node, 2^42 per unit charge number (exact, order-free) */
    /* full EM only; lattice arrays are 4 per node: E = (Ex(i+1/2,j,k), Ey(i,j+1/2,k), Ez(i,j,k+1/2), 0), B on the faces */
    FPIC_F3_B_NODES = 4,   /* out: node-centred B, 4 per node */
    FPIC_F3_EDGE_E = 5,    /* in: value[i][j][k][3]; out: 4 per node */
    FPIC_F3_FACE_B = 6,    /* in: value[i][j][k][3]; out: 4 per node */
    FPIC_F3_J_FIXED = 7    /* out: 3 int64 per node (x-, y-, z-edge), 96 * 2^42 per particle crossing a dual face: with RHO_FIXED the
                              lattice continuity equation 96 (rho^(n+1) - rho^n) + div J = 0 holds exactly */
} fpic_field3;

/* Device buffers whose address can be handed to a collective (see fpic_device_buffer). */
typedef enum fpic_buffer {
    FPIC_BUF_CELL_SUMS = 0, /* per-cell sums 0.001*(vr,vtheta,vz,1), (nr+11)*(nz+11)*4 scalars: sprite-centre cell (ic, jc),
                               ic in -5..nr+5, at 4*((ic+5) + (nr+11)*(jc+5)); opaque to a host that only sums it over ranks */
    FPIC_BUF_RHO_FIXED = 1  /* CART3D: int64 charge accumulators, nr*ny*nz */
} fpic_buffer;

/*
 * Construction parameters.  The first eight fields are the reference's spec
 * (empic.js:31-41, all 'number').  `nparticles` is the side of the reference's
 * particle texture: the particle count is nparticles*nparticles (empic.js:107-109)
 * unless `count` is non-zero (extension).
 */
typedef struct fpic_spec {
    double radius;          /* m */
    double height;          /* m */
    int32_t nr;
    int32_t nz;
    double dt;              /* s, fixed for the life of the handle (empic.js:44, :852) */
    int32_t nparticles;     /* texture side; count = nparticles^2 */
    double particle_mass;   /* kg */
    double particle_charge; /* C  */
    /* ---- extensions (zero = reference behaviour) ---- */
    uint64_t count;         /* exact particle count overriding nparticles^2 */
    int32_t precision;      /* fpic_dtype of the device state; reference is F32 */
    int32_t device;         /* HIP device ordinal */
    int32_t physical_a;     /* 0: reference's K9 formula incl. quirk Q1 (empic.js:645);
                               1: h(E.B)B vector form */
    int32_t sort_interval;  /* re-bin particles every k density() calls; 0 = adaptive */
    int32_t unfused_deposit;/* 0: step() also forms the per-cell sums of density()'s scatter, counts
                               particles per tile and re-bins them (the frame loop of
                               fusionsim.js:172-174 always calls density() after step());
                               1: separate passes for all of that;
                               2: census and re-binning stay in step(), the sums are a separate pass
                               (faster with rng_mode 1, where no gather hides the LDS atomics) */
    int32_t rng_mode;       /* 0: the reference's generator (entropy-table walk K3, per-particle state,
                               empic.js:783-820).  1: counter-based extension: the random
                               vector of particle i at sub-step t is Philox4x32-10(counter (i, t, 0x5EED),
                               key rng_seed); no per-particle random state, no entropy table */
    uint32_t rng_seed_lo, rng_seed_hi;
    int32_t geometry;       /* fpic_geometry; 0 = the reference's (r,z) pusher */
    int32_t solver;         /* fpic_solver (CART3D) */
    int32_t ny;             /* CART3D: nodes along y (nr along x, nz along z) */
    int32_t shape;          /* fpic_shape of density() on the (r,z) grid; CART3D always deposits CIC */
    double length_y;        /* CART3D: box is radius (x) x length_y x height (z) metres */
    double macro_weight;    /* CART3D: real particles per macro-particle (charge density scale); 0 = 1 */
    int32_t raster_subpixel_bits; /* density()'s point sprites (empic.js:980-1035, :1473-1478) on the (r,z) grid.
                               0: ideal sprites — window coordinates of infinite precision, a point whose centre lies
                               outside the clip volume is discarded whole (the GL ES 2.0 text).
                               b = 1..8: as a rasteriser with b sub-pixel bits draws them — window position snapped to
                               2^-b pixel (round half to even, y running downwards), left/top edges inclusive, a point whose
                               centre has left the target cropped instead of discarded.  b = 4 reproduces the reference
                               run under Chromium's ANGLE/SwiftShader bit for bit (tests/golden/webgl_*); desktop GPUs
                               usually have 8.  Only the cell a particle's 11x11 stamp is centred on changes (one cell
                               lower for a coordinate within 2^-(b+1) pixel above a pixel edge).  Carved out of the
                               former reserved[6]: same size and offsets, ABI unchanged */
    int32_t bin_lookahead;  /* (r,z) push: the re-binning files a particle in the tile of position + k sub-steps of its
                               velocity instead of the tile it is in, so that over a binning period it drifts from -k to
                               period - k sub-steps away from its bin instead of from 0 to the period.  Speed only:
                               no result depends on the bins.
                               0: default — adaptive (half the last period plus one launch, at most 64 sub-steps) when
                               sort_interval == 0, none when sort_interval > 0;  -1: off in every mode;  k > 0: k sub-steps
                               in every mode.
                               The first binning and fpic_sort always key on the position.  Carved out of the former
                               reserved_i32: same size and offsets, ABI unchanged */
    double reserved[5];
} fpic_spec;

typedef struct fpic_handle fpic_handle;

/* Counters and timings; all times are HIP-event milliseconds on the handle's stream
 * and are gathered only while profiling is enabled (fpic_profile). */
typedef struct fpic_stats {
    uint64_t n_particles;
    uint64_t particle_updates;   /* sub-steps x particles since create */
    uint64_t step_launches;      /* push kernel launches */
    uint64_t deposit_launches;
    uint64_t sort_passes;
    uint64_t deposit_spilled;    /* particles of the last deposit that missed their LDS tile */
    double ms_push;              /* sum over push launches */
    double ms_deposit;           /* sum over cell-sum (scatter) launches */
    double ms_stamp;             /* sum over stamp-convolution + normalise + EMA launches */
    double ms_precalc;
    double ms_sort;
    uint64_t bytes_particle_state; /* device bytes held for particle state */
    uint64_t bytes_grid_state;
    double ms_solve;             /* CART3D: sum over field solves (rho conversion, FFTs, k-space, gradient) */
    uint64_t solve_launches;
    uint64_t outbox_items;       /* (r,z) re-binning launches: work items whose leavers went through the outbox */
    uint64_t outbox_full_items;  /* ... and work items that found no room in it and stored their leavers directly */
    double reserved[4];
} fpic_stats;

/* Last error text.  h may be NULL after a failed fpic_create. */
const char* fpic_last_error(const fpic_handle* h);

/* Library/ABI version, and the code-object architecture it was built for ("gfx950"). */
int fpic_abi_version(void);
const char* fpic_build_arch(void);

/* empic.makeCylindricalParticlePusher(spec): validation (empic.js:31-41,
 * utilities.js:118-127), derived constants h, factor_r, factor_z (empic.js:44-46),
 * all state buffers (empic.js:123-241, :499-502, :666-672, :933-1072), the 11x11
 * stamp (empic.js:949-971). */
int fpic_create(const fpic_spec* spec, fpic_handle** out);
int fpic_destroy(fpic_handle* h);

/* out.set({position, velocity}) (empic.js:1199-1244).  pos/vel are AoS [n][3] in
 * metres / units of c, dtype F32 or F64; either may be NULL.  n must equal the
 * handle's particle count.  Normalisation by factor_r, factor_r, factor_z is done
 * in double and rounded once, as the reference's Float32Array store does. */
int fpic_set_particles(fpic_handle* h, const void* pos_aos, const void* vel_aos, uint64_t n, int dtype);

/* out.set({E, B, sink_mask, source_pdf}) (empic.js:1159-1197, :1246-1349).
 * data is value[i][j][k] flattened, i over nr, j over nz, k over ncomp (3 or 1). */
int fpic_set_grid(fpic_handle* h, int which, const void* data, int nr, int nz, int ncomp, int dtype);

/* Reproducible replacement for window.crypto / Math.random (empic.js:142-180, quirk
 * Q8): entropy is 1024*1024*4 floats (index 4*(i + 1024*j)), rand is n*4 floats
 * (u1,u2,c1,c2).  Either may be NULL to keep the current one. */
int fpic_set_random_state(fpic_handle* h, const float* entropy, const float* rand);

/* Static field painters, additive into B (empic.js:1352-1363, :1380-1411). */
int fpic_add_current_loop(fpic_handle* h, double r, double z, double current);
int fpic_add_current_z(fpic_handle* h, double current);
int fpic_add_bz(fpic_handle* h, double bz);
int fpic_add_btheta(fpic_handle* h, double btheta);

/* out.precalc() (empic.js:1413-1434): B,E -> R1,R2,R3,A. */
int fpic_precalc(fpic_handle* h);

/* out.step() (empic.js:1436-1469) ncalls times; each call is two leap-frog
 * sub-steps (RandB,VelB,PosB,RandA,VelA,PosA). */
int fpic_step(fpic_handle* h, int ncalls);
/* The same advance counted in single leap-frog sub-steps: fpic_step(h, n) == fpic_substeps(h, 2 n).  The reference can
 * only advance in pairs (empic.js:1436-1469 draws both halves of the ping-pong); an odd count exists for diagnostics that
 * need the state between the two halves (the continuity check of the full-EM cycle, a sampled comparison with the oracle
 * in a field read back beforehand). */
int fpic_substeps(fpic_handle* h, int nsub);

/* out.density() (empic.js:1471-1495): scatter (K4), normalise (K5), EMA (K6),
 * avgB <- avgA (K7).  fpic_density == fpic_deposit then fpic_density_finish; the
 * split exists so that a multi-GPU host can sum FPIC_BUF_CELL_SUMS across ranks
 * in between. */
int fpic_density(fpic_handle* h);
int fpic_deposit(fpic_handle* h);
int fpic_density_finish(fpic_handle* h);
/* fpic_density_finish reading the per-cell sums from a caller's device buffer (same layout as
 * FPIC_BUF_CELL_SUMS) and running on a caller's stream (NULL: the handle's).  A multi-GPU host
 * copies the sums out after fpic_deposit, all-reduces the copy and finishes from it on a side
 * stream while the next step() already runs; the library orders its own later reads of the
 * density grids after that finish. */
int fpic_density_finish_from(fpic_handle* h, const void* sums, void* hip_stream);

/* fb.readPixels (utilities.js:701-711) for the grids above.  out holds
 * 4*W*H floats (dtype F32) or doubles (F64). */
int fpic_read_grid(fpic_handle* h, int which, void* out, int dtype);

/* Particle read-back in the caller's original order (normalised units as stored:
 * x/R, y/R, z/H and v/c scaled the same way).  pos_aos/vel_aos are [n][3] of
 * dtype, rand is [n][4] float, alive is [n] bytes; any may be NULL. */
int fpic_get_particles(fpic_handle* h, void* pos_aos, void* vel_aos, float* rand, uint8_t* alive, int dtype);

/* NGP cell index i + j*nr of every particle as the push sees it (integer parity
 * check; same order as fpic_get_particles). */
int fpic_get_cells(fpic_handle* h, int32_t* cells);

/* Multi-GPU plumbing: the raw device address/byte size of a buffer (for an RCCL
 * collective issued by the host), and the HIP stream the handle enqueues on.
 * fpic_set_stream(h, NULL) restores the handle's own stream. */
int fpic_device_buffer(fpic_handle* h, int which, void** dptr, size_t* bytes);
int fpic_set_stream(fpic_handle* h, void* hip_stream);
int fpic_get_stream(fpic_handle* h, void** hip_stream);

/* ---- CART3D extension entry points (FPIC_ERR_STATE on an (r,z) handle) ---- */
/* A further species sharing the grid (the reference has one species per pusher, empic.js:37-38).
 * charge must be a non-zero integer multiple (|Z| <= 255) of spec.particle_charge; the macro weight
 * is shared.  *index receives the species number (spec's own species is 0). */
int fpic_add_species(fpic_handle* h, double mass, double charge, uint64_t count, int* index);
int fpic_set_particles_of(fpic_handle* h, int species, const void* pos_aos, const void* vel_aos, uint64_t n, int dtype);
/* the caller's particles [first, first + n) of a species: populations too large for one host array are
 * uploaded piecewise (2e9 particles are 48 GB of AoS floats).  pos_aos / vel_aos here and in
 * fpic_domain_set_particles may be host OR device memory (copied with hipMemcpyDefault on the handle's stream;
 * for device memory the caller has synchronised whatever produced it). */
int fpic_set_particles_range(fpic_handle* h, int species, uint64_t first, uint64_t n, const void* pos_aos, const void* vel_aos, int dtype);
int fpic_get_particles_of(fpic_handle* h, int species, void* pos_aos, void* vel_aos, int dtype);
int fpic_get_cells_of(fpic_handle* h, int species, int32_t* cells);
/* The mirror of fpic_set_particles_range, and a sampled read-back: the caller's particles first, first + stride,
 * first + 2 stride, ... — n of them (stride >= 1; stride 1 = the contiguous range [first, first + n)) — in the caller's
 * order, pos_aos / vel_aos [n][3] of dtype (either may be NULL).  The reference can only display its particles
 * (fusionsim.js:174-178; utilities.js:701-711 has readPixels, unused): 2e9 particles are 48 / 96 GB of host arrays, so a
 * host reads them piecewise or samples them (every 20 000th particle of BASELINE configs[4] for the oracle comparison). */
int fpic_get_particles_range(fpic_handle* h, int species, uint64_t first, uint64_t n, uint64_t stride, void* pos_aos, void* vel_aos, int dtype);
int fpic_get_cells_range(fpic_handle* h, int species, uint64_t first, uint64_t n, uint64_t stride, int32_t* cells);
/* uniform external B (T), additive like the reference's painters (empic.js:1391-1400) */
int fpic_add_b(fpic_handle* h, double bx, double by, double bz);
/* which = FPIC_F3_E only: value[i][j][k][3] flattened, dims must equal the handle's */
int fpic_set_field3(fpic_handle* h, int which, const void* data, int nx, int ny, int nz, int dtype);
/* out: nodes (RHO, PHI), 4*nodes (E) of dtype, or nodes int64 (RHO_FIXED, dtype ignored) */
int fpic_read_field3(fpic_handle* h, int which, void* out, int dtype);

/* ---- multi-GPU inside the library (the reference has one WebGL context and no
 * communication).  One process per GPU, one handle per process; the library binds RCCL at run time and
 * issues the collectives itself, so the JavaScript host needs no other collective library.
 *   rank 0: fpic_comm_unique_id(id); the host hands the 128 bytes to every rank (file, socket, env);
 *   every rank: fpic_comm_init(h, id, rank, world).
 * (r,z) pusher, reference-parity mode: each rank holds a shard of the particles (contiguous index range)
 * and a replica of the grid tables; fpic_density then sums FPIC_BUF_CELL_SUMS over the ranks with ONE
 * all-reduce between the scatter and the stamp stage — by default on a side stream, off the critical path
 * of the next fpic_step (fpic_comm_set_overlap(h, 0) keeps it on the handle's stream). */
#define FPIC_UNIQUE_ID_BYTES 128
int fpic_comm_unique_id(void* id128);
int fpic_comm_init(fpic_handle* h, const void* id128, int rank, int world);
int fpic_comm_destroy(fpic_handle* h);
int fpic_comm_info(fpic_handle* h, int* rank, int* world);
int fpic_comm_set_overlap(fpic_handle* h, int enable);

/* ---- CART3D spatial decomposition: z-slabs.  spec describes the GLOBAL box and grid on
 * every rank; spec.count is the rank's CAPACITY per species.  Rank r of `world` owns the particles whose cell lies
 * in the planes [r nz/world, (r+1) nz/world); they may sit up to ghost_planes planes outside it between two
 * migrations (every migrate_every sub-steps).  Per sub-step the ranks exchange: the ghost planes of the int64
 * charge grid with their two neighbours (added exactly), then an all-gather of the owned planes of rho; every rank
 * then solves the fields.  At a migration: two counts and two particle messages (6 scalars + the caller's global
 * index) per neighbour, grouped ncclSend/ncclRecv.  Because the charge grid is an integer grid, an N-rank run
 * reproduces the one-GPU run bit for bit.
 *   with a communicator (fpic_comm_init, one process per GPU): fpic_precalc / fpic_step exchange over RCCL;
 *   fpic_group_precalc / fpic_group_step: all `n` ranks are handles of THIS process on one device and the exchange
 *   is device-to-device copies — the stand-in that lets one GPU run and test an N-rank decomposition. */
/* distributed_solve = 0: every rank gathers rho and transforms the whole grid (the N-rank run is then bit-identical to one GPU);
 * 1: the Poisson solve is decomposed too — 2-D transforms of the owned planes, an all-to-all transposition (each pair of ranks
 * exchanges nz/N * ny/N * (nx/2+1) complex values), transforms along z on ny/N rows, the transposition back, and G+1 / G+2 planes
 * of the potential from the neighbours: no rank touches the whole grid, fields agree with one GPU to rounding (needs ny % N == 0).
 * On power-of-two grids (the library's own transforms) the decomposed solve is the one handle's bit for bit, full-EM handles
 * take it for their initial field as well, and the rank then KEEPS ONLY ITS SLAB: nz/N + 2 (ghost_planes + 2) + 1 planes of
 * every node array instead of nz (FPIC_DOMAIN_COMPACT=0 keeps whole-grid arrays).  Call it on a fresh handle: node fields
 * uploaded before it are dropped (upload after).  fpic_read_field3 still fills a whole-grid-shaped array: the planes the
 * rank holds in their places, zero elsewhere; fpic_device_buffer(FPIC_BUF_RHO_FIXED) is then the held planes only.
 * 2: decomposed WITHOUT the transpositions (power-of-two grids, up to 8 ranks): K^2 = k2x + k2y + k2z with k2z the eigenvalues
 * of the three-point second difference, so after the x and y transforms of its own planes every (kx, ky) mode is a periodic
 * tridiagonal system along z; each rank eliminates its nz/N planes to a two-equation interface, ONE all-gather carries two
 * planes of the half spectrum per rank (1/32 of the transpositions' bytes at nz/N = 64), every rank solves the 2N-unknown
 * interface system of each mode redundantly and substitutes back (csrc/fes_tri.hpp).  Equal to the transform solve in exact
 * arithmetic: fields agree with one GPU to rounding (2e-5 / 1e-10), not bit for bit.  Slab-only arrays as with 1. */
int fpic_domain_init(fpic_handle* h, int rank, int world, int ghost_planes, int migrate_every, int distributed_solve);
/* the rank's initial particles (positions anywhere in its slab +- ghost planes); their global indices are first_id, first_id+1, ... */
int fpic_domain_set_particles(fpic_handle* h, int species, uint64_t n, const void* pos_aos, const void* vel_aos, uint32_t first_id, int dtype);
/* the particles the rank holds now, in no particular order, with their global indices; *n receives the count
 * (pass NULL buffers to query it) */
int fpic_domain_get_particles(fpic_handle* h, int species, void* pos_aos, void* vel_aos, uint32_t* ids, uint64_t capacity, uint64_t* n, int dtype);
int fpic_domain_stats(fpic_handle* h, uint64_t* migrated, uint64_t* lost);
int fpic_group_precalc(fpic_handle** handles, int n);
int fpic_group_step(fpic_handle** handles, int n, int ncalls);
/* out.density() (empic.js:1471) of every member of a full-EM group: the charge grid of the current positions, complete on
 * every member's own planes (ghost planes exchanged and added).  Over a communicator every rank calls fpic_density. */
int fpic_group_density(fpic_handle** handles, int n);

/* Counter-based RNG mode only: the global sub-step index (starts at 0, +2 per step() call);
 * settable so that a run can be resumed. */
int fpic_get_substep_counter(fpic_handle* h, uint64_t* t);
int fpic_set_substep_counter(fpic_handle* h, uint64_t t);

/* Force a re-bin of the particle arrays by cell tile now (normally automatic). */
int fpic_sort(fpic_handle* h);

/* Read-back / resume (the reference can only display its state,
 * utilities.js:701-711 is unused): a flat binary dump of the particle arrays in the caller's
 * order and of the grid tables, and its inverse.  The target handle of a load must have been
 * created from the same spec.  A run resumed from a checkpoint continues bit-identically.
 * A box (spec.geometry = CART3D) saves the raw state of every species and its fields (its own file layout); the
 * target handle must have the same species added.  A rank of a decomposition writes / reads its own file (the particles
 * it holds with their global indices; full EM: the lattice fields of its planes; the electrostatic field is recomputed
 * by fpic_precalc after the load). */
int fpic_save_checkpoint(fpic_handle* h, const char* path);
int fpic_load_checkpoint(fpic_handle* h, const char* path);

/* ---- CART3D energy and momentum diagnostics, reduced on the device (the oracle's field_energy, em_field_energy and
 * kinetic_energy; the reference has no counterpart).  Sums are accumulated in double whatever the precision of the state,
 * in a fixed order (no float atomics): the same state gives the same bits. */
#define FPIC_ENERGY_SPECIES 16          /* = the decomposition's species limit; a box with more species gets FPIC_ERR_STATE */
typedef struct fpic_energy {
    uint64_t substep;                   /* sub-steps this handle has advanced since create when the values were taken */
    int32_t  nspecies, reserved_i32;
    double   field_e;                   /* J: 0.5 eps0 sum |E|^2 dV.  Electrostatic: node E (E4.xyz); full EM: the lattice E */
    double   field_b;                   /* J: 0.5/mu0 sum |B|^2 dV of the lattice B at the integer time (full EM; 0 otherwise),
                                           with the uniform external part included, as oracle em_field_energy */
    double   field_b_external;          /* J: 0.5/mu0 |B0|^2 dV over the nodes summed (full EM; 0 otherwise): the external part of
                                           field_b.  A rank counts its own planes, so the ranks' sum counts the box volume once */
    uint64_t count[FPIC_ENERGY_SPECIES];
    double   kinetic[FPIC_ENERGY_SPECIES];      /* J: 0.5 m W c^2 sum |v|^2 of the stored velocities (as oracle kinetic_energy) */
    double   momentum[FPIC_ENERGY_SPECIES][3];  /* kg m/s: m W c sum v */
    double   speed_max[FPIC_ENERGY_SPECIES];    /* max |v| in units of c */
    double   reserved[8];
} fpic_energy;
/* The particle sums are exact: every term (|v|^2, vx, vy, vz of a stored velocity, in double) is floored once to a multiple
 * of 2^-80 (c^2 or c) and the integers are added in 128 bits, so the result does not depend on the particles' order; the
 * sum is then rounded once to the nearest double.  A velocity that is not finite, or a term of 2^15 or more (|v| >= 181 c),
 * cannot enter such a sum: the species' kinetic is then NaN, so is each momentum component that met one, and speed_max is
 * NaN (a |v|^2 was NaN) or +inf.  The other species are unaffected. */

#define FPIC_DIAG_LOCAL  0   /* this handle's particles and the planes it owns */
#define FPIC_DIAG_GLOBAL 1   /* the whole simulation; with a communicator this is collective (every rank calls it) */

/* Enqueues the reduction on the handle's stream, waits, fills *out.  GLOBAL on a decomposed handle without a communicator
 * (a member of an in-process group) is FPIC_ERR_STATE: the host adds up the members' LOCAL values. */
int fpic_energy_now(fpic_handle* h, int scope, fpic_energy* out);
/* After every `every`-th sub-step the same reduction is enqueued behind the sub-step and its row written into a device ring
 * of `capacity` rows: no host synchronisation, no collective.  every = 0 turns recording off and frees the ring; a new
 * call starts an empty ring. */
int fpic_energy_record(fpic_handle* h, int every, uint32_t capacity);
/* The rows recorded since the last drain, oldest first (rows = NULL: *n receives how many there are, nothing is drained).
 * If the ring wrapped, the newest `capacity` rows are returned and *dropped counts the others.  GLOBAL with a communicator
 * is collective: every rank must hold the same number of rows (else FPIC_ERR_STATE on every rank). */
int fpic_energy_history(fpic_handle* h, int scope, fpic_energy* rows, uint64_t capacity, uint64_t* n, uint64_t* dropped);

/* ---- CART3D phase-space histograms, reduced on the device: the live particles of ONE species binned over one or two axes,
 * without reading a particle back.  The value q of an axis is a double made from the particle's state in normalised units
 * as stored (what fpic_get_particles_of / fpic_domain_get_particles return in the handle's own precision):
 *   FPIC_AXIS_X, _Y, _Z     the stored position, a fraction of the box in [0, 1), converted to double
 *   FPIC_AXIS_VX, _VY, _VZ  the stored velocity in units of c, converted to double.  Full EM (solver = YEE): the stored
 *                           velocity is the half-time one of the leap-frog, and it is binned as stored
 *   FPIC_AXIS_V2            vx*vx + vy*vy + vz*vz in double, added left to right, every operation rounded once
 * Per axis the caller gives bins >= 1 and finite lo < hi; scale = bins / (hi - lo) is formed once, in double.  A particle
 *   is INSIDE the axis iff q >= lo && q < hi (a NaN is not inside), and its index there is
 *   k = min((int64) floor((q - lo) * scale), bins - 1)   (subtraction and product each rounded once, no fused multiply-add;
 *                                                          the min only catches a product that rounds up to bins).
 * A particle inside every axis adds 1 to counts[k0] (one axis) or counts[k0 * bins[1] + k1] (two axes, row-major
 * [bins[0]][bins[1]], the layout of numpy.histogram2d); every other live particle adds 1 to *outside.  So
 * sum(counts) + *outside = fpic_energy.count[species] always.  The dead slots of a decomposed rank are skipped.  Counts are
 * integers added with integer atomics: the same state gives the same bits.
 * Refused (FPIC_ERR_INVALID_ARG): naxes other than 1 or 2, a species the handle does not have, an axis code outside 0..6,
 * the same axis twice, bins < 1, bins[0] * bins[1] above FPIC_HIST_MAX_BINS, lo / hi not finite or not lo < hi or with a
 * bins / (hi - lo) that is not finite, a reserved word that is not zero; a handle that is not CART3D.  precalc() is not
 * needed: the call reads particles only. */
#define FPIC_AXIS_X  0
#define FPIC_AXIS_Y  1
#define FPIC_AXIS_Z  2
#define FPIC_AXIS_VX 3
#define FPIC_AXIS_VY 4
#define FPIC_AXIS_VZ 5
#define FPIC_AXIS_V2 6
#define FPIC_HIST_MAX_BINS (1u << 22)   /* 32 MiB of counters */
typedef struct fpic_hist_spec {
    int32_t species, naxes;      /* naxes 1 or 2 */
    int32_t axis[2], bins[2];    /* FPIC_AXIS_X .. FPIC_AXIS_V2 */
    double  lo[2], hi[2];
    double  reserved[4];         /* zero */
} fpic_hist_spec;
/* counts: bins[0] (* bins[1]) words; outside: one word.  scope as for fpic_energy_now: LOCAL is this handle's own particles;
 * GLOBAL with a communicator is collective (every rank calls it with the same spec and gets the same sums); GLOBAL on a
 * member of an in-process group is FPIC_ERR_STATE (the host adds up the members' LOCAL counts).  Synchronous: enqueues on
 * the handle's stream, copies back, waits. */
int fpic_histogram(fpic_handle* h, const fpic_hist_spec* spec, int scope, uint64_t* counts, uint64_t* outside);

/* ---- CART3D fluid moment grids, reduced on the device: the velocity moments of order 0, 1 and 2 of ONE species on the node
 * grid, as exact int64 sums, without reading a particle back.  Ten moments, one bit of `mask` each; the particle value m
 * is a double made from the stored velocity in units of c converted to double (full EM, solver = YEE: the half-time
 * velocity as stored, as in fpic_histogram):
 *   bit 0       N             1
 *   bits 1 2 3  FX FY FZ      vx, vy, vz
 *   bits 4 5 6  SXX SYY SZZ   vx*vx, vy*vy, vz*vz     (one multiplication in double, rounded once)
 *   bits 7 8 9  SXY SXZ SYZ   vx*vy, vx*vz, vy*vz     (likewise)
 * Per live particle (the dead slots of a decomposed rank are skipped): the cell (i, j, k) and the upper weights wx1, wy1,
 * wz1 (0 .. 16384) are those of the charge deposit, formed from the stored position in the handle's precision; the lower
 * weight is w0 = 16384 - w1, the eight nodes are (i+a, j+b, k+c), a, b, c in {0, 1}, wrapped periodically.
 *   REJECTED: a particle with a velocity component that is not finite or has |v| >= 128 adds to NO moment (not to N either)
 *     and adds 1 to info->rejected.  So every |m| < 2^14 and no integer below overflows.
 *   N adds wx[a] * wy[b] * wz[c] to node (a, b, c): 2^42 per particle — the charge deposit's integer with Z = 1, so the sum
 *     over the species of Z_s * N_s equals FPIC_F3_RHO_FIXED bit for bit.
 *   Every other moment: t = (int64) floor(m * 2^32) (the scaling is exact; one floor, also for a negative m).  t is split
 *     with remainder axis by axis, z first, then y, then x:  upper = (w1 * t + 8192) >> 14 (an arithmetic, flooring shift),
 *     lower = t - upper.  t -> (tz[0], tz[1]) by wz1; each tz[c] -> (tzy[c][0], tzy[c][1]) by wy1; each of those -> the
 *     terms of nodes a = 0, 1 by wx1; index 1 is the upper part.  The eight terms of a particle add up to t exactly:
 *     summed over the nodes, a moment equals the sum of t over the accepted particles, and N equals 2^42 times their number.
 * Accumulators are int64 per node and moment, node index i + nr * (j + ny * k), added as two's-complement integer atomics:
 * the same state gives the same bits whatever the slot order, the binning, the tile shape or the number of ranks.  A node
 * holds 2^21 unit-weight particles of N before overflow (the bound of rho_fixed with Z = 1); |t| < 2^46 leaves the other
 * moments at least 2^17 particles of the largest value per node.
 * out: popcount(mask) grids of nr * ny * nz int64 each, in ascending bit order.
 * scope as for fpic_histogram.  LOCAL is the contribution of THIS HANDLE'S OWN PARTICLES: on a rank of a decomposition the
 *   grids are whole-grid-shaped, the planes the rank holds (its slab and the ghost / halo planes) in their places and zero
 *   elsewhere.  A rank's particles in its ghost planes add to nodes the rank does not own — that is intended: the ranks'
 *   LOCAL grids are partial sums that add up, as integers, to exactly the grids of one undecomposed handle.  GLOBAL with a
 *   communicator is collective (every rank calls it with the same spec; the grids and both counters are summed over the
 *   ranks, every rank gets the same full grids); GLOBAL on a member of an in-process group is FPIC_ERR_STATE (the host adds
 *   up the members' LOCAL grids).
 * info->spilled counts the accepted particles that added through global memory instead of their tile's window in LDS (a
 *   particle that has left its tile since the last binning; every particle of a species that is not binned); it has no
 *   effect on the sums.
 * Refused (FPIC_ERR_INVALID_ARG): a null pointer, a species the handle does not have, mask == 0, bits above 9, a reserved
 * word that is not zero; FPIC_ERR_STATE: a handle that is not CART3D.  precalc() is not needed; the call reads particles and
 * writes nothing but its own buffer.  Synchronous: enqueues on the handle's stream, copies back, waits. */
#define FPIC_MOM_N   (1u << 0)
#define FPIC_MOM_FX  (1u << 1)
#define FPIC_MOM_FY  (1u << 2)
#define FPIC_MOM_FZ  (1u << 3)
#define FPIC_MOM_SXX (1u << 4)
#define FPIC_MOM_SYY (1u << 5)
#define FPIC_MOM_SZZ (1u << 6)
#define FPIC_MOM_SXY (1u << 7)
#define FPIC_MOM_SXZ (1u << 8)
#define FPIC_MOM_SYZ (1u << 9)
#define FPIC_MOM_ORDER0 0x001u
#define FPIC_MOM_ORDER1 0x00Fu
#define FPIC_MOM_ORDER2 0x3FFu
typedef struct fpic_moments_spec {
    int32_t  species;
    uint32_t mask;
    double   reserved[4];        /* zero */
} fpic_moments_spec;
typedef struct fpic_moments_info {
    uint64_t rejected;           /* particles left out by the rule above */
    uint64_t spilled;            /* particles that added through global memory; no effect on the sums */
    uint64_t reserved[2];
} fpic_moments_info;
int fpic_moments(fpic_handle* h, const fpic_moments_spec* spec, int scope, int64_t* out, fpic_moments_info* info);

/* ---- CART3D series: the field at chosen points and the state of chosen particles (tracers) as rows of doubles, taken now
 * or recorded after every `every`-th sub-step into a device ring, without reading a grid or a species back.  One request
 * holds two lists, either of which may be empty (not both):
 *   points[npoints][3]   positions in metres, anywhere: a point outside [0, L) is wrapped periodically
 *   tracers[ntracers]    pairs (tracer_species[t], tracer_id[t]); the id is the caller's particle index within the species
 *                        (first + k of fpic_set_particles_range / fpic_get_particles_range; on a decomposed handle the
 *                        first_id + k of fpic_domain_set_particles, what fpic_domain_get_particles returns as ids)
 * A POINT ROW is 8 doubles: the four components of the node record FPIC_F3_E (Ex, Ey, Ez and the fourth as stored: phi in the
 * electrostatic box), the three of FPIC_F3_B_NODES (zeros unless solver = YEE), and `present` (1.0 or 0.0).  The value is
 * interpolated from exactly the arrays fpic_read_field3 returns for those two grids at that moment (reading them closes
 * nothing and forms nothing), with the charge deposit's weights:
 *   1. per axis u = p / L in double, u -= floor(u), u = 0 if that is not < 1; then u is converted to the handle's precision T;
 *   2. the cell i and the upper weight w1 (0 .. 16384) are the charge deposit's, evaluated in T:
 *      g = u * n, i = (int) g (i = 0 if that is n), w1 = ((int) ((g - floor(g)) * 32768) + 1) >> 1;  w0 = 16384 - w1;
 *   3. the eight nodes (i+a, j+b, k+c), a, b, c in {0, 1}, wrapped periodically, e = a + 2 b + 4 c, with the integer weight
 *      W_e = wx[a] * wy[b] * wz[c] (they add up to 2^42);
 *   4. per component value = (sum over e of (double) W_e * (double) F_e) * 2^-42: the first product starts the sum, the other
 *      seven are added in the order e = 1 .. 7, every operation rounded once in double, no fused multiply-add.
 * A point on a node therefore gets the node's record exactly (one weight is 2^42, the others 0), as long as u * n lands
 * within 2^-16 of the integer (in float: up to 64 nodes per axis).
 * A TRACER ROW is 8 doubles: the six stored numbers of the particle — position as a fraction of the box, velocity in units
 * of c, each converted to double, what fpic_get_particles_range / fpic_domain_get_particles return with dtype f64 —, `found`
 * (1.0 or 0.0) and a zero.  A handle reports the tracers whose LIVE slot it holds (the dead slots of a decomposed rank never
 * match).  An entry that is not present / not found is all zeros.
 * scope: LOCAL is what this handle sees.  On a rank of a z-slab decomposition a point belongs to the rank that owns plane k
 * of step 2; that rank must hold the plane above its slab too (ghost_planes >= 1; FPIC_ERR_STATE otherwise).  GLOBAL with a
 * communicator is collective: the ranks' rows are gathered and every rank takes each entry from the rank whose flag is set
 * (a selection, not a sum; two flags for one entry are FPIC_ERR_STATE).  GLOBAL on a member of an in-process group is
 * FPIC_ERR_STATE (the host selects among the members' LOCAL rows).
 * Refused (FPIC_ERR_INVALID_ARG): a null pointer, both lists empty, more than FPIC_SERIES_MAX_POINTS points or
 * FPIC_SERIES_MAX_TRACERS tracers, a point that is not finite, a species the handle does not have, the same (species, id)
 * twice, on an undecomposed handle an id that is not below the species' count (a decomposed rank accepts any id: it does not
 * know the total), a reserved word that is not zero, capacity = 0 with every > 0; FPIC_ERR_STATE: a handle that is not
 * CART3D, points before fpic_precalc. */
#define FPIC_SERIES_MAX_POINTS  4096u
#define FPIC_SERIES_MAX_TRACERS 65536u
typedef struct fpic_series_spec {
    uint32_t        npoints, ntracers;
    const double*   points;          /* [npoints][3], metres */
    const int32_t*  tracer_species;  /* [ntracers] */
    const uint32_t* tracer_id;       /* [ntracers] */
    double          reserved[4];     /* zero */
} fpic_series_spec;
/* The rows of the current state: points_out [npoints][8], tracers_out [ntracers][8] (either may be NULL when its list is
 * empty).  Enqueues on the handle's stream, copies back, waits.  fpic_precalc is needed only if npoints > 0. */
int fpic_series_now(fpic_handle* h, const fpic_series_spec* spec, int scope, double* points_out, double* tracers_out);
/* After every `every`-th sub-step (the counter of fpic_energy.substep) the same rows are written into a device ring of
 * `capacity` rows on the handle's stream: no host synchronisation, no collective.  every = 0 turns recording off and frees
 * the ring (spec may then be NULL); a new call starts an empty ring.  Independent of fpic_energy_record. */
int fpic_series_record(fpic_handle* h, const fpic_series_spec* spec, int every, uint32_t capacity);
/* The rows recorded since the last drain, oldest first: substeps[r], points_out[r][npoints][8], tracers_out[r][ntracers][8]
 * for r < *n (substeps = NULL: *n receives how many there are, nothing is drained).  capacity: the rows the arrays have room
 * for.  If the ring wrapped, the newest rows are returned and *dropped counts the others.  GLOBAL with a communicator is
 * collective: every rank must hold the same number of rows (else FPIC_ERR_STATE on every rank). */
int fpic_series_history(fpic_handle* h, int scope, uint64_t* substeps, double* points_out, double* tracers_out, uint64_t capacity,
                        uint64_t* n, uint64_t* dropped);

/* ---- CART3D modes: the complex Fourier amplitudes of the node fields at a chosen list of wave vectors, taken now or
 * recorded after every `every`-th sub-step into a device ring, without reading a grid back and without a full transform (any
 * grid shape).  A request names nmodes wave vectors m = (mx, my, mz) as int32 triples and a mask of quantities:
 *   FPIC_MODE_EX, _EY, _EZ, _PHI   the four components of the node record FPIC_F3_E as stored (the fourth is phi in the
 *                                  electrostatic box)
 *   FPIC_MODE_BX, _BY, _BZ         the three components of FPIC_F3_B_NODES (all zero unless solver = YEE, as in a point row)
 *   FPIC_MODE_RHO                  the integer charge grid FPIC_F3_RHO_FIXED converted to double, times the double
 *                                  q0 W / (2^42 dV) with which the library forms FPIC_F3_RHO (formed as
 *                                  particle_charge * macro_weight / (4398046511104.0 * dV), dV = (lx/nx) * (ly/ny) * (lz/nz))
 * The arrays are read as they are at that moment — nothing is closed and nothing is formed, exactly as a point row of
 * fpic_series reads them — so the amplitude is the discrete transform of what a point series on every node would return.
 * For a quantity F on the N = nx ny nz nodes (node index i + nx * (j + ny * k)):
 *   A(m) = (1/N) * sum_k sum_j sum_i (double) F[k][j][i] * wx[(mx i) mod nx] * wy[(my j) mod ny] * wz[(mz k) mod nz]
 * The arithmetic is double in fp32 and fp64 states alike (a float converts exactly).  (m i) mod n is integer arithmetic; a
 * negative m is reduced into [0, n) first.  wa[t] = exp(-2 pi i t / na) comes from three tables of doubles built on the
 * host with two guaranteed properties: an entry with 4 t divisible by na is exactly (+-1, 0) or (0, +-1), and wa[na - t] is
 * bit for bit the conjugate of wa[t] (t <= na / 2 is computed, the rest mirrored).  So a field of small integers at modes
 * whose twiddles all lie in {+-1, +-i} sums exactly, and A(-m) is exactly conj A(m).
 * The order of the sum is fixed — a function of the grid shape, the planes the handle owns and the request alone.  With p
 * the smallest power of two >= nmodes and S = 256 / p: the owned rows (k, j), in the order of j + ny * k, are cut into
 * contiguous shares of ceil(rows / 1024) rows, one per workgroup.  Within a share, for each s < S: per row the terms of
 * the nodes i = s, s + S, s + 2 S, ... are added in ascending i (product F * wx first, re and im apart), that sum is
 * multiplied by (wy * wz) of the row, and the rows' products are added in row order; then the S sums are added in the
 * order s = 0, 1, ...  The workgroups' sums are added in workgroup order within 64 contiguous groups of
 * ceil(workgroups / 64), the groups' sums in group order, and the total is divided by N.  Every operation is rounded once
 * (no fused multiply-add).  So the order depends on nmodes through S, and on nothing else of the request: a permuted list
 * and any sub-mask return the same bits for what they share, a request with another NUMBER of modes returns another
 * rounding of the same sums.  No floating-point atomics; no dependence on timing: two calls on one state, and two handles
 * holding the same fields, return the same bits.
 * out: double [nmodes][nq][2] (re, im), the nq selected quantities in ascending bit order.
 * scope: LOCAL is the sum over the planes this handle owns (all nz; the slab of a rank of a decomposition), with k the
 * global plane and N the global node count, so the ranks' LOCAL rows add up to the box.  GLOBAL with a communicator is
 * collective: the ranks' rows are gathered and added in rank order on every rank (every rank gets the same bits).  GLOBAL on
 * a member of an in-process group is FPIC_ERR_STATE (the host adds up the members' LOCAL rows in rank order).
 * Refused (FPIC_ERR_INVALID_ARG): a null pointer, nmodes = 0 or above FPIC_MODES_MAX, a component outside [-na/2, na/2],
 * the same triple twice, an empty mask or unknown bits, a reserved word that is not zero, capacity = 0 with every > 0;
 * FPIC_ERR_STATE: a handle that is not CART3D, a call before fpic_precalc, a rank that does not hold its owned planes.
 * The recorder is not part of a checkpoint (as the series' and the energy's are not): arm it again after a load. */
#define FPIC_MODES_MAX 256u
#define FPIC_MODE_EX  (1u << 0)
#define FPIC_MODE_EY  (1u << 1)
#define FPIC_MODE_EZ  (1u << 2)
#define FPIC_MODE_PHI (1u << 3)
#define FPIC_MODE_BX  (1u << 4)
#define FPIC_MODE_BY  (1u << 5)
#define FPIC_MODE_BZ  (1u << 6)
#define FPIC_MODE_RHO (1u << 7)
#define FPIC_MODE_ALL 0xFFu
typedef struct fpic_modes_spec {
    uint32_t        nmodes, mask;
    const int32_t*  modes;           /* [nmodes][3] */
    double          reserved[4];     /* zero */
} fpic_modes_spec;
/* The amplitudes of the current state: out [nmodes][nq][2].  Enqueues on the handle's stream, copies back, waits. */
int fpic_modes_now(fpic_handle* h, const fpic_modes_spec* spec, int scope, double* out);
/* After every `every`-th sub-step (the counter of fpic_energy.substep) the same row is written into a device ring of
 * `capacity` rows on the handle's stream: no host synchronisation, no collective.  every = 0 turns recording off and frees
 * the ring (spec may then be NULL); a new call starts an empty ring; a refused call leaves the running recorder as it was.
 * Independent of fpic_energy_record and fpic_series_record. */
int fpic_modes_record(fpic_handle* h, const fpic_modes_spec* spec, int every, uint32_t capacity);
/* The rows recorded since the last drain, oldest first: substeps[r], out[r][nmodes][nq][2] for r < *n (substeps = NULL: *n
 * receives how many there are, nothing is drained).  capacity: the rows the arrays have room for.  If the ring wrapped, the
 * newest rows are returned and *dropped counts the others.  GLOBAL with a communicator is collective: every rank must hold
 * the same number of rows (else FPIC_ERR_STATE on every rank). */
int fpic_modes_history(fpic_handle* h, int scope, uint64_t* substeps, double* out, uint64_t capacity, uint64_t* n, uint64_t* dropped);

/* ---- CART3D particle selection, filtered and compacted on the device: the live particles of ONE species that lie in a
 * window of phase space (and, optionally, whose id falls in a residue class) handed to the caller as ids, positions and
 * velocities, without reading the species back.  A request holds nterms (0 .. FPIC_SELECT_MAX_TERMS) terms, each an axis
 * code with a half-open interval [lo, hi):
 *   the value q of an axis is exactly fpic_histogram's: FPIC_AXIS_X .. _VZ the stored number converted to double (positions
 *   as fractions of the box in [0, 1), velocities in units of c; full EM: the stored half-time velocity as it is),
 *   FPIC_AXIS_V2 vx*vx + vy*vy + vz*vz in double, added left to right, every operation rounded once.
 * A live particle MATCHES a term iff q >= lo && q < hi, compared in double (a NaN matches nothing).  Unlike the histogram's
 * bounds, lo may be -inf and hi may be +inf; a NaN bound, or a pair that is not lo < hi, is refused.  A particle is SELECTED
 * iff it is live, matches every term and passes the id rule: id_mod 0 or 1 passes every id, otherwise only ids with
 * id % id_mod == id_rem.  The dead slots of a decomposed rank are never selected.  nterms = 0 selects every live particle
 * (subject to the id rule).  A window across the periodic boundary is two calls.
 * The id is the one the tracer series uses: the caller's particle index on an undecomposed handle (first + k of
 * fpic_set_particles_range), the global id on a decomposed rank (first_id + k of fpic_domain_set_particles).
 * Outputs: *matched is always the number of selected particles.  If matched <= capacity, rows [0, matched) of ids,
 * pos_aos ([row][3]) and vel_aos ([row][3]) are written IN ASCENDING ID — the same state gives the same bytes —, the values
 * being the stored ones cast to `dtype` with a C cast; bytes past `matched` rows are untouched; any of the three pointers
 * may be NULL.  If matched > capacity nothing is written to the arrays and the call still returns FPIC_OK: capacity = 0
 * with all pointers NULL is the count query (the two-call idiom of fpic_series_history).
 * scope: LOCAL is this handle's particles.  GLOBAL with a communicator is collective (every rank calls it with the same
 * request and capacity): matched is the sum over the ranks, and if it fits every rank receives the same rows, merged in
 * ascending id.  GLOBAL on a member of an in-process group is FPIC_ERR_STATE (the host merges the members' LOCAL rows).
 * Refused (FPIC_ERR_INVALID_ARG): a null spec or matched, nterms outside 0 .. 7, an axis code outside 0 .. 6, the same axis
 * twice, a NaN bound or not lo < hi, id_rem >= id_mod when id_mod > 1, a reserved word that is not zero, entries past
 * nterms that are not zero, a species the handle does not have, capacity above FPIC_SELECT_MAX_ROWS, capacity > 0 with all
 * three pointers NULL, a dtype that is neither F32 nor F64; FPIC_ERR_STATE: a handle that is not CART3D.  precalc() is not needed: the call
 * reads particles and writes nothing but its own buffer.  Synchronous: enqueues on the handle's stream, copies back, waits. */
#define FPIC_SELECT_MAX_TERMS 7
#define FPIC_SELECT_MAX_ROWS  (1u << 24)
typedef struct fpic_select_spec {
    int32_t  species, nterms;   /* nterms 0..7; 0: every live particle (subject to the id rule) */
    int32_t  axis[8];           /* FPIC_AXIS_X .. FPIC_AXIS_V2, each code at most once; zero past nterms */
    double   lo[8], hi[8];
    uint32_t id_mod, id_rem;    /* id_mod 0 or 1: every id; otherwise only ids with id % id_mod == id_rem */
    double   reserved[4];       /* zero */
} fpic_select_spec;
int fpic_select(fpic_handle* h, const fpic_select_spec* spec, int scope, uint64_t capacity,
                uint32_t* ids, void* pos_aos, void* vel_aos, int dtype, uint64_t* matched);

/* ---- CART3D particle loader: a population generated on the device, without host arrays.  The state of particle i (the
 * caller's index = the id the box carries) depends on the request and on i alone — not on the slot, the rank of a
 * decomposition, the precision of the handle or the time of the call.  All arithmetic is double, every operation rounded
 * once; an fp32 handle stores the float rounding of the same double result.
 *   words      W(b) = Philox4x32-10(counter (i, stream, b, 0x10AD), key (seed lo, seed hi)); b = 0 positions, b = 1
 *              velocities; the lattice shifts are the block with counter (0, stream, 2, 0x10AD).  Two species loaded with the
 *              same seed and stream get identical states; different streams are independent.
 *   fractions  default (FPIC_LOAD_RANDOM)  f_a = W(0)[a] 2^-32
 *              FPIC_LOAD_LATTICE           f_a = ((i mult_a + shift_a) mod 2^32) 2^-32, mult = 3518319155, 2882110345,
 *                                          2360945575 (a Kronecker lattice), shift_a = word a of the shift block
 *   position   in box fractions: p_a = lo[a]/L_a + f_a (hi[a] - lo[a])/L_a (one multiply, one add); the phase in turns
 *              theta = (mode[0] p_x + mode[1] p_y) + mode[2] p_z; p_a += xamp[a]/L_a sinpi(2 (theta + xphase)); stored as
 *              the upload stores it (cast to the handle's precision, wrapped into [0, 1)).
 *   velocity   in units of c: Box-Muller on W(1) = (w0, w1, w2, w3): u1 = (w0 + 0.5) 2^-32, u2 = w1 2^-32,
 *              n0 = sqrt(-2 ln u1) cospi(2 u2), n1 = sqrt(-2 ln u1) sinpi(2 u2),
 *              n2 = sqrt(-2 ln((w2 + 0.5) 2^-32)) cospi(2 w3 2^-32) (|n| <= 6.76);
 *              v_a = drift[a] + vth[a] n_a + vamp[a] sinpi(2 (theta + vphase)), theta from the undisplaced p.
 *   FPIC_LOAD_PAIRED  the velocity block is taken at i & ~1 and the thermal term of odd i is negated: with zero drift and
 *              vamp the thermal momentum of an even-aligned, even-length range is exactly zero.
 * An undecomposed handle: particles [first, first + count) of the species (count = ~0: to the end) are written where they
 * are now — before the first binning or in the middle of a run —, every other particle keeps its bits; FPIC_LOAD_POS /
 * FPIC_LOAD_VEL choose the arrays written (at least one).  *loaded = count.
 * A rank of a decomposition (after fpic_domain_init): the indices [first, first + count) are global ids; the rank generates
 * them all and KEEPS those whose cell plane floor(z nz) it owns, in ascending id, so the ranks of a world hold between them
 * exactly the particles one handle would, bit for bit.  Both arrays are required and count must be given.  The call
 * replaces the rank's population of the species (as fpic_domain_set_particles); with FPIC_LOAD_APPEND the kept particles
 * follow those the rank holds (several ranges, e.g. two beams; before the first step or after fpic_sort).  If the kept
 * particles exceed the species' capacity on this rank the call returns FPIC_ERR_INVALID_ARG and changes nothing.
 * *loaded = the particles kept.  Not collective.
 * After a load that wrote positions the fields are stale, as after fpic_set_particles_range: fpic_precalc comes next.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, a species the handle does not have, a range outside the species, neither POS
 * nor VEL, unknown flag bits, a reserved word that is not zero, a value that is not finite, vth < 0, not
 * 0 <= lo < hi <= L, |mode[a]| > 2^15; FPIC_ERR_STATE: a handle that is not CART3D.  Synchronous. */
#define FPIC_LOAD_RANDOM  0u   /* positions from the random words (the default) */
#define FPIC_LOAD_POS     1u
#define FPIC_LOAD_VEL     2u
#define FPIC_LOAD_LATTICE 4u   /* positions from the Kronecker lattice */
#define FPIC_LOAD_PAIRED  8u
#define FPIC_LOAD_APPEND  16u
typedef struct fpic_load_spec {
    int32_t  species;
    uint32_t flags;
    uint64_t first, count;      /* count = ~0: to the end of the species (an undecomposed handle) */
    uint64_t seed;
    uint32_t stream, reserved;  /* reserved: zero */
    double   lo[3], hi[3];      /* the sub-box in metres, 0 <= lo < hi <= L */
    double   drift[3], vth[3];  /* units of c */
    int32_t  mode[3], reserved2;
    double   xamp[3], xphase;   /* metres; turns */
    double   vamp[3], vphase;   /* units of c; turns */
} fpic_load_spec;
int fpic_load(fpic_handle* h, const fpic_load_spec* spec, uint64_t* loaded);

/* ---- CART3D particle loader with profiles: fpic_load with tabulated, separable profiles along the axes for the density,
 * the thermal speed and one drift component.  Every flag and field of the request keeps its meaning, and so does what the
 * state of particle i depends on: the request, the tables and i alone.  A null profile, or one whose node counts are all
 * zero, is fpic_load bit for bit.
 * A table of n nodes is uniformly spaced over the request's sub-box on its axis — node 0 at lo[a], node n - 1 at hi[a] —
 * and linear between the nodes.  K = n - 1 is its number of intervals.  All arithmetic is double, every operation rounded
 * once, and every operation of a position is one of + - * / sqrt.
 *   density    C[0] = 0, C[j+1] = C[j] + 0.5 (d[j] + d[j+1]), summed in sequence on the host.  With f the unit fraction
 *              fpic_load draws on that axis (random or lattice):
 *                  t = f C[K];  j = the largest index with C[j] <= t, held to K - 1;  r = t - C[j];
 *                  disc = d[j] d[j] + (2 (d[j+1] - d[j])) r, held to 0 from below;  den = d[j] + sqrt(disc);
 *                  s = den > 0 ? (2 r) / den : 0, held to 1 from above;
 *                  f' = (j + s) / K, and 1 - 2^-53 if that is not below 1.
 *              An interval without mass is never chosen.  p_a = lo[a]/L_a + f' (hi[a] - lo[a])/L_a; theta, the
 *              displacement, the cast and the wrap are fpic_load's.  An axis without a table has f' = f.  A lattice load
 *              becomes a quiet start on the profile; a PAIRED load or two species on one stream stay exactly neutral.
 *   lookup     a thermal or shear table of K intervals at the fraction f' of its axis: g = f' K; j = min((int) g, K - 1);
 *              s = g - j; value = tab[j] + (tab[j+1] - tab[j]) s.
 *   velocity   vth_eff[a] = ((vth[a] sx) sy) sz with sx, sy, sz the thermal tables' values at the UNDISPLACED position (a
 *              missing table is a factor of exactly 1: no multiply); drift_eff[c] = drift[c] + shear(f' of shear_axis) for
 *              c = shear_component; then fpic_load's velocity with vth_eff and drift_eff.
 * Refused (FPIC_ERR_INVALID_ARG) besides what fpic_load refuses: a node count of 1 or above FPIC_LOAD_TABLE_MAX, a null
 * table whose count is not zero, a value that is not finite, a negative density or thermal value, a density table whose
 * total is 0, shear_axis or shear_component outside 0..2, a reserved word that is not zero.  Synchronous. */
#define FPIC_LOAD_TABLE_MAX 1025          /* nodes of one table */
/* (a struct tag, not a typedef: the tables and the call share the name as `struct stat` and stat() do, so the type is
 * written `struct fpic_load_profile` in C and in C++) */
struct fpic_load_profile {
    uint32_t density_n[3];                /* nodes per axis: 0 = uniform, else 2 .. FPIC_LOAD_TABLE_MAX */
    uint32_t thermal_n[3];                /* 0 = factor 1 */
    uint32_t shear_n;                     /* 0 = none */
    int32_t  shear_axis, shear_component; /* 0..2 each: drift[component] += table(position along axis) */
    uint32_t reserved[2];                 /* zero */
    const double* density[3];             /* >= 0, finite, at least one interval with mass */
    const double* thermal[3];             /* >= 0, finite: multiplies vth[0..2] */
    const double* shear;                  /* finite, units of c */
};
int fpic_load_profile(fpic_handle* h, const fpic_load_spec* spec, const struct fpic_load_profile* profile, uint64_t* loaded);

/* ---- CART3D particle loader with radial profiles: a spherical or a cylindrical population whose density, thermal speed and
 * flows are tables of the radius — a hot spot in a shell with an implosion velocity, a pinch with an axial drift, a rotating
 * column.  Every flag and field of the request keeps its meaning (lo and hi only on the cylinder's own axis), and so does
 * what the state of particle i depends on: the request, the tables and i alone.
 * A table of n nodes is uniformly spaced over [0, r_max] — node 0 on the centre (the axis), node n - 1 at r_max — and linear
 * between the nodes.  K = n - 1 is its number of intervals, rho the radius in units of r_max.  All arithmetic is double,
 * every operation rounded once; the radius takes only + - * / and comparisons.  f0, f1, f2 are the unit fractions fpic_load
 * draws on the three axes (random or lattice).
 *   mass       in units of the node spacing, with d0 = d[j], D = d[j+1] - d[j], J = (double) j, the mass of interval j up to
 *              the place s in [0, 1], in Horner form ("x s" multiplies the sum so far by s, "a + (..)" adds a to it):
 *                sphere (weight rho^2)    JJ = J J;  a1 = d0 JJ;  a2 = d0 J + 0.5 (D JJ);  a3 = (d0 + (2 J) D) / 3;  a4 = 0.25 D;
 *                                         M_j(s) = (a1 + (a2 + (a3 + a4 s) s) s) s
 *                cylinder (weight rho)    a1 = d0 J;  a2 = 0.5 (d0 + D J);  a3 = D / 3;
 *                                         M_j(s) = (a1 + (a2 + a3 s) s) s
 *              C[0] = 0, C[j+1] = C[j] + M_j(1), summed in sequence on the host, M_j(1) by the same evaluation at s = 1.
 *   radius     f = f0 for the sphere, the fraction of axis b for the cylinder:
 *                  t = f C[K];  j = the largest index with C[j] <= t, held to K - 1;  r = t - C[j];
 *                  lo = 0, hi = 1; 52 times: mid = 0.5 (lo + hi); if M_j(mid) <= r then lo = mid, else hi = mid;  s = lo;
 *                  rho = (J + s) / K, and 1 - 2^-53 if that is not below 1.
 *              An interval without mass is never chosen.  density_n = 0 is the table {1, 1}: uniform in the volume (the
 *              area).  A lattice load is a quiet start on the profile.
 *   direction  sphere:    mu = 2 f1 - 1;  q = sqrt(1 - mu mu);  cs = cospi(2 f2), sn = sinpi(2 f2);  dir = (q cs, q sn, mu).
 *              cylinder about axis a, with b = (a + 1) mod 3 and c = (a + 2) mod 3:
 *                         dir_a = 0, dir_b = cospi(2 f_c), dir_c = sinpi(2 f_c).
 *   position   in box fractions: p_k = center[k]/L_k + (rho (r_max/L_k)) dir_k; along the cylinder's axis fpic_load's own
 *              p_a = lo[a]/L_a + f_a (hi[a] - lo[a])/L_a.  theta, the displacement, the cast and the wrap are fpic_load's: a
 *              body that reaches across the periodic boundary wraps.
 *   velocity   the tables are read by fpic_load_profile's lookup at f' = rho (of the UNDISPLACED position).
 *              vth_eff[k] = vth[k] thermal(rho) (no table: a factor of exactly 1, no multiply);
 *              sphere:    drift_eff[k] = drift[k] + u_r dir_k
 *              cylinder:  drift_eff[a] = drift[a] + u_a;  drift_eff[b] = (drift[b] + u_r dir_b) + u_t (-dir_c);
 *                         drift_eff[c] = (drift[c] + u_r dir_c) + u_t dir_b
 *              with u_r, u_t, u_a the radial, azimuthal and axial tables' values (a flow without a table adds nothing);
 *              then fpic_load's velocity with vth_eff and drift_eff.
 * Refused (FPIC_ERR_INVALID_ARG) besides what fpic_load refuses: a null request, an unknown geometry, an axis outside 0..2
 * (a sphere: other than 0), r_max that is not positive and finite, 2 r_max above the box length on an axis the body spans
 * (the sphere: all three, the cylinder: the two across its axis), a centre outside [0, L], a node count of 1 or above
 * FPIC_LOAD_TABLE_MAX, a null table whose count is not zero, a value that is not finite, a negative density or thermal
 * value, a density table whose total mass is 0, azimuthal_n or axial_n for the sphere, a reserved word that is not zero.
 * FPIC_ERR_STATE: a handle that is not CART3D.  Synchronous. */
#define FPIC_LOAD_SPHERE   1u
#define FPIC_LOAD_CYLINDER 2u
struct fpic_load_radial {                 /* (a tag, as struct fpic_load_profile) */
    uint32_t geometry;                    /* FPIC_LOAD_SPHERE or FPIC_LOAD_CYLINDER */
    int32_t  axis;                        /* the cylinder's axis 0..2; a sphere: 0 */
    double   center[3], r_max;            /* metres; the cylinder ignores center[axis] */
    uint32_t density_n, thermal_n, radial_n, azimuthal_n, axial_n;   /* nodes; 0 = none (density: uniform in volume) */
    uint32_t reserved[3];                 /* zero */
    const double* density;                /* >= 0, finite, at least one interval with mass */
    const double* thermal;                /* >= 0, finite: multiplies vth */
    const double* radial;                 /* finite, units of c: the flow along dir */
    const double* azimuthal;              /* the cylinder: the flow about the axis */
    const double* axial;                  /* the cylinder: the flow along the axis */
};
int fpic_load_radial(fpic_handle* h, const fpic_load_spec* spec, const struct fpic_load_radial* radial, uint64_t* loaded);

/* ---- CART3D Monte Carlo collisions with a prescribed background: a drifting Maxwellian (drift, vth per axis, units of c)
 * that is not another species; the momentum and energy the species loses go to that reservoir.  The operator acts on the
 * stored velocities of one species (under full EM the half-time velocity, as fpic_histogram reads it), as a call or
 * registered to run after every k-th sub-step.  What happens to particle i (the id the box carries) depends on the request,
 * the epoch, i and its stored velocity alone — not on the slot, the binning or the rank; with sigma_tau = 0 WHO collides
 * does not depend on the precision of the handle either.  All arithmetic is double, every operation rounded once; a stored
 * velocity is converted to double and the result cast back to the handle's precision.
 *   words      W(b) = Philox4x32-10(counter (i, epoch, stream, 0xC0110 + b), key (seed lo, seed hi)), the loader's
 *              generator.  W(0) = (w0, w1, w2, w3): candidate, acceptance, two direction words; W(1): the partner's
 *              three normals n, by the loader's Box-Muller formulas on the four words.
 *   numbers    x_max = nu_tau + sigma_tau g_max; P_max = -expm1(-x_max); K = (uint64) ldexp(P_max, 32) (x_max = +inf:
 *              K = 2^32); M = mass_ratio / (1 + mass_ratio) (+inf: M = 1); RELAX: decay = exp(-nu_tau),
 *              sv[a] = sqrt(-expm1(-2 nu_tau)) vth[a].
 *   candidate  (EXCHANGE, ELASTIC) a live particle with (uint64) w0 < K — an integer comparison.
 *   partner    vb[a] = drift[a] + vth[a] n[a]; d[a] = v[a] - vb[a]; g = sqrt((d0 d0 + d1 d1) + d2 d2).
 *   acceptance sigma_tau == 0: every candidate collides.  Otherwise (null-collision method) x = nu_tau + sigma_tau
 *              min(g, g_max), u = (w1 + 0.5) 2^-32, and the candidate collides iff u x_max < x; a candidate with g > g_max
 *              is also counted as `clipped`: the caller's bound was too low.
 *   EXCHANGE   (charge exchange, Krook) v' = vb.
 *   ELASTIC    (isotropic in the centre-of-mass frame) c = 1 - 2 (w2 + 0.5) 2^-32, s = sqrt(1 - c c), phi = w3 2^-32,
 *              nhat = (s cospi(2 phi), s sinpi(2 phi), c); per component t = g nhat[a], r = d[a] - t, q = M r,
 *              v'[a] = v[a] - q.
 *   RELAX      (the exact Ornstein-Uhlenbeck step of the Lenard-Bernstein operator) no candidates: every live particle is
 *              updated and counted as `collided`; r = v[a] - drift[a], p = decay r, k = sv[a] n[a], q = p + k,
 *              v'[a] = drift[a] + q.
 * A particle that does not collide keeps its bits; positions are never written, so the fields stay valid and fpic_precalc
 * is not needed.  A dead slot of a rank of a decomposition is never a candidate and never counted.
 * fpic_collide applies the request now (synchronous) and returns its counts (applications = 1; with K = 0 nothing can
 * collide: all four are zero and nothing runs).  fpic_collide_register makes it run at the end of every sub-step whose
 * number (counted since create) is a multiple of `every`, in registration order, before the recorders take their rows —
 * a row recorded after that sub-step sees the collided state — with epoch (uint32)(sub-step + spec.epoch): a resumed run
 * passes the sub-steps already done.  The count is the handle's own: on a resumed handle the phase of `every` starts again,
 * so a run cut at a sub-step that is not a common multiple of the registered periods cannot be reproduced by its resumption
 * (cut at one, it continues bit for bit: tests/test_gpu_sequences.py).  At most FPIC_COLLIDE_MAX_OPS operators; *index names the operator.  Nothing is
 * synchronised: the counts accumulate on the device and fpic_collide_stats reads the totals since registration (scope as
 * for the diagnostics: GLOBAL with a communicator sums candidates, collided and clipped over the ranks; applications is the
 * same on every rank and is not summed).  fpic_collide_clear drops every registered operator.  Registrations are not part of
 * a checkpoint.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, an unknown kind, a species the handle does not have, a NaN anywhere, a
 * negative rate, sigma_tau not finite, vth < 0 or not finite, a drift that is not finite, g_max not (> 0 and finite) with
 * sigma_tau > 0 or not 0 without, nu_tau = +inf with sigma_tau > 0, mass_ratio given for a kind other than ELASTIC or <= 0
 * for ELASTIC, RELAX with sigma_tau != 0, nu_tau == 0 or nu_tau = +inf, a reserved word that is not zero, every < 1, a
 * ninth registration, an index outside the registered operators; FPIC_ERR_STATE: a handle that is not CART3D. */
#define FPIC_COLLIDE_EXCHANGE 0
#define FPIC_COLLIDE_ELASTIC  1
#define FPIC_COLLIDE_RELAX    2
#define FPIC_COLLIDE_MAX_OPS  8
typedef struct fpic_collide_spec {
    int32_t  species, kind;        /* FPIC_COLLIDE_EXCHANGE 0, _ELASTIC 1, _RELAX 2 */
    uint64_t seed;
    uint32_t stream, epoch;
    double   nu_tau;               /* nu tau >= 0, +inf allowed (not for RELAX) */
    double   sigma_tau;            /* n sigma c tau >= 0, finite; per unit of g */
    double   g_max;                /* > 0 and finite when sigma_tau > 0, else 0 */
    double   drift[3], vth[3];     /* the background, units of c; vth >= 0 */
    double   mass_ratio;           /* m_background / m_species > 0, +inf allowed; ELASTIC only, else 0 */
    double   reserved[4];          /* zero */
} fpic_collide_spec;
typedef struct fpic_collide_result { uint64_t applications, candidates, collided, clipped; } fpic_collide_result;
int fpic_collide(fpic_handle* h, const fpic_collide_spec* spec, fpic_collide_result* out);
int fpic_collide_register(fpic_handle* h, const fpic_collide_spec* spec, int every, int* index);
int fpic_collide_stats(fpic_handle* h, int index, int scope, fpic_collide_result* out);
int fpic_collide_clear(fpic_handle* h);

/* ---- CART3D binary Coulomb collisions between the species of the box (Takizuka & Abe 1977): species_a with species_b,
 * species_a == species_b for like-particle collisions.  The particles of a grid cell are paired at random and every pair is
 * scattered by a small random angle; the operator acts on the stored velocities (under full EM the half-time velocity), as
 * a call or registered to run after every k-th sub-step.  The result depends on the request, the epoch, the particles'
 * ids, their cells and their stored velocities alone — not on the slots, the binning or the order the kernels visit
 * anything in.  All arithmetic is double, every operation rounded once; a stored velocity is converted to double, and
 * AFTER EVERY PAIR both velocities are cast back to the handle's precision: a particle's next pair starts from the cast
 * value.  Velocities are in units of c.
 *   cell       the charge deposit's cell (i, j, k) of the stored position, evaluated in the handle's precision as the
 *              deposit and fpic_moments do.
 *   words      P(b) = Philox4x32-10(counter (id, epoch, stream, 0xC0120 + b), key (seed lo, seed hi)), the loader's
 *              generator.
 *   order      the particles of one species in a cell are sorted ascending by (P(0)[0] of their own id, id).
 *   numbers    m_ab = m_a m_b / (m_a + m_b); kappa = (q_a q_b)^2 log_lambda tau W / (8 pi eps0^2 m_ab^2 c^3 dV), dV the
 *              cell volume as in the charge density's scale, W the macro weight, eps0 and c the constants of the box
 *              (8.8541878128e-12, 2.998e8); the mass factors m_ab / m_a and m_ab / m_b.
 *   unlike     Nm >= Nf the two counts in the cell, `many` the species with more particles (a tie: species_a).  Nf = 0:
 *              nothing.  many[j] pairs with few[j mod Nf]; a few particle takes its partners in ascending j; the owner of a
 *              pair is the many particle; N_L = Nf.
 *   like       N particles s[0 .. N).  N < 2: nothing.  N even: the pairs (s[2t], s[2t+1]), the owner the first member,
 *              N_L = N.  N odd: (s0,s1), (s1,s2), (s2,s0) in that order, each owner the first member, with N_L = N / 2
 *              (a double: half the variance), then the pairs (s[3+2t], s[4+2t]) with N_L = N.
 *   one pair   (owner o, partner p) u = v_o - v_p; up = sqrt(ux ux + uy uy); g = sqrt((ux ux + uy uy) + uz uz).  g == 0: the
 *              pair is unchanged and not counted.  var = (kappa N_L) / ((g g) g); var > 1 is also counted as `strong` (tau is
 *              too long for small-angle theory; the pair is still collided).  delta = sqrt(var) n0, n0 the first normal of
 *              the loader's Box-Muller formulas on P(1) of o.  d2 = delta delta; sinT = (2 delta) / (1 + d2);
 *              omc = (2 d2) / (1 + d2); phi = P(0)[1] of o 2^-32; cs = cospi(2 phi), sn = sinpi(2 phi).  With up > 0,
 *              ex = ux / up, ey = uy / up:
 *                  dux = ((((ex uz) sinT) cs) - (((ey g) sinT) sn)) - ux omc
 *                  duy = ((((ey uz) sinT) cs) + (((ex g) sinT) sn)) - uy omc
 *                  duz = (-((up sinT) cs)) - uz omc
 *              with up == 0: du = ((g sinT) cs, (g sinT) sn, -(g omc)).
 *              v_o' = v_o + (m_ab / m_o) du; v_p' = v_p - (m_ab / m_p) du.
 * A cell holding more than FPIC_PAIR_CELL_MAX particles of either species is not collided: it is counted in overfull_cells
 * and its particles (both species) in overfull_particles, and every one of them keeps its bits.  Positions are never
 * written: the fields stay valid, the bin tables and the census stay as they are, fpic_precalc is not needed.
 * fpic_pair applies the request now (synchronous) and returns its counts: applications = 1, pairs (the pairs with g != 0),
 * strong, cells (the cells that had a pair to collide), overfull_cells, overfull_particles.  fpic_pair_register makes it
 * run at the end of every sub-step whose number (counted since create) is a multiple of `every`, after the operators of
 * fpic_collide_register and before the recorders take their rows, in registration order, with epoch
 * (uint32)(sub-step + spec.epoch).  The count is the handle's own: on a resumed handle the phase of `every` starts again, so
 * a resume point must be a common multiple of the registered periods, and the resumed registration passes the sub-steps
 * already done in spec.epoch.  At most FPIC_PAIR_MAX_OPS operators; *index names the operator.  Nothing is
 * synchronised: the counts accumulate on the device and fpic_pair_stats reads the totals since registration.
 * fpic_pair_clear drops every registered pair operator (those of fpic_collide_register stay).  Registrations are not part
 * of a checkpoint.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, a species the handle does not have, a NaN anywhere, log_lambda or tau not
 * (> 0 and finite), a reserved word that is not zero, every < 1, a ninth registration, an index outside the registered
 * operators; FPIC_ERR_STATE: a handle that is not CART3D, and a handle with a domain decomposition (between two migrations
 * the particles of a cell can sit on two ranks, in the ghost planes: a rank cannot pair a cell alone). */
#define FPIC_PAIR_MAX_OPS  8
#define FPIC_PAIR_CELL_MAX 2048
typedef struct fpic_pair_spec {
    int32_t  species_a, species_b;
    uint64_t seed;
    uint32_t stream, epoch;
    double   log_lambda;           /* the Coulomb logarithm, > 0 and finite */
    double   tau;                  /* s: the time one application stands for, > 0 and finite */
    double   reserved[4];          /* zero */
} fpic_pair_spec;
typedef struct fpic_pair_result { uint64_t applications, pairs, strong, cells, overfull_cells, overfull_particles; } fpic_pair_result;
int fpic_pair(fpic_handle* h, const fpic_pair_spec* spec, fpic_pair_result* out);
int fpic_pair_register(fpic_handle* h, const fpic_pair_spec* spec, int every, int* index);
int fpic_pair_stats(fpic_handle* h, int index, int scope, fpic_pair_result* out);
int fpic_pair_clear(fpic_handle* h);

/* ---- CART3D fusion yield tally: the number of binary reactions between species_a and species_b of the box (species_a ==
 * species_b: a species with itself, D-D) in the time tau, per grid cell and in total, from a tabulated cross-section.  It is a
 * TALLY, NOT A SINK: it reads the stored velocities and writes nothing to any particle; reactants are not consumed and no
 * products are made.  The result depends on the request, the epoch, the particles' ids, their cells and their stored
 * velocities alone — not on the slots, the binning or the order the kernels visit anything in.  All arithmetic is double,
 * every operation one of + - x / sqrt and rounded once; the sums are integers, so they are exact.  Velocities are in units
 * of c.
 *   cell, order, pairs   exactly those of fpic_pair above (the deposit's cell; ascending by (key, id); unlike species
 *              many[j] with few[j mod Nf], N_L = Nf, Nm pairs; like species the pairs (s[2t], s[2t+1]) with N_L = N, an odd
 *              cell's leading triple (s0,s1), (s1,s2), (s2,s0) with N_L = N / 2), but the key is
 *              Philox4x32-10(counter (id, epoch, stream, 0xF0510), key (seed lo, seed hi))[0]: a tag of its own, so a tally
 *              never correlates with a Coulomb operator on the same seed.
 *   one pair   u = v_o - v_p; g = sqrt((ux ux + uy uy) + uz uz).
 *   the table  n values sigma[k] (m^2, 2 <= n <= FPIC_FUSION_TABLE_MAX, each finite and >= 0) at relative speeds uniform in
 *              g: g_k = g_lo + k dg, dg = (g_hi - g_lo) / (n - 1), 0 <= g_lo < g_hi finite.  g < g_lo is counted `below`,
 *              g >= g_hi is counted `above`; both contribute nothing.  Otherwise t = (g - g_lo) inv_dg with
 *              inv_dg = (n - 1) / (g_hi - g_lo), k = min(floor(t), n - 2), sigma = sigma[k] + (t - k) (sigma[k+1] - sigma[k]),
 *              held to max sigma (a guard of the last rounding).  With E = m_ab (g c)^2 / 2, 4096 points over 1 keV .. 1 MeV
 *              (a speed ratio of 32) resolve the low end to better than 1 %.
 *   yield      y = ((((W W) N_L) tau) / dV) (sigma (g c)) real reactions, W the macro weight, dV the cell volume, c =
 *              2.998e8.  Unlike species: the pairs of a cell add to W^2 Na Nb <sigma v> tau / dV; like species: the pair
 *              weights add to N^2 / 2.
 *   fixed point   y_bound = ((((W W) 2048) tau) / dV) (max sigma (g_hi c)); unit_exponent e = the smallest integer with
 *              y_bound < 2^(e + 40) (not below -1000); a pair adds q = (int64) floor(y 2^-e) < 2^40 to its cell's word of
 *              the grid and to the total.  The grid is nz x ny x nx int64, x fastest, in units of 2^e reactions; the total
 *              is yield_hi 2^32 + yield_lo in the same unit (yield_lo < 2^32).  A cell receives fewer than 2^51 per
 *              application, so a registered operator's grid is exact for at least 4096 applications between two drains
 *              (fpic_fusion_grid with reset); nothing detects an overflow beyond that.
 * A cell holding more than FPIC_PAIR_CELL_MAX particles of either species is skipped: it is counted in overfull_cells and its
 * particles (both species) in overfull_particles.  A table whose entries are all zero launches nothing; every count but
 * `applications` is zero and unit_exponent is 0.
 * fpic_fusion tallies now (synchronous) and returns the counts — applications = 1, pairs (those inside the table), below,
 * above, cells (the cells that had a pair), overfull_cells, overfull_particles, yield_hi, yield_lo, unit_exponent — and, if
 * `grid` is not NULL, the nz*ny*nx cell words.  fpic_fusion_register copies the table and makes the tally run at the end of
 * every sub-step whose number (counted since create) is a multiple of `every`, after the operators of fpic_pair_register
 * (it sees the collided velocities) and before the recorders, in registration order, with epoch
 * (uint32)(sub-step + spec.epoch); its grid and totals accumulate on the device with no host synchronisation.  At most
 * FPIC_FUSION_MAX_OPS operators; *index names the operator.  fpic_fusion_stats reads the totals since registration (or since
 * the last reset), fpic_fusion_grid copies the operator's grid (grid may be NULL with reset != 0) and, with reset != 0,
 * zeroes the grid, the totals and `applications` behind the copy in stream order.  fpic_fusion_clear drops every registered
 * tally.  Registrations are not part of a checkpoint.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, a species the handle does not have, a reserved word that is not zero, tau
 * not (> 0 and finite), n outside 2 .. 4096, a null table, g_lo < 0 or not finite, g_hi <= g_lo or not finite, a table entry
 * that is negative or not finite, a yield bound that is not finite, every < 1, a fifth registration, an index outside the
 * registered operators, fpic_fusion_grid with neither a grid nor reset; FPIC_ERR_STATE: a handle that is not CART3D, and a
 * handle with a domain decomposition (as fpic_pair: a rank cannot pair a cell alone). */
#define FPIC_FUSION_MAX_OPS   4
#define FPIC_FUSION_TABLE_MAX 4096
typedef struct fpic_fusion_spec {
    int32_t  species_a, species_b;
    uint64_t seed;
    uint32_t stream, epoch;
    double   tau;                  /* s: the time one application stands for, > 0 and finite */
    double   g_lo, g_hi;           /* units of c: the table's first and last relative speed */
    int32_t  n, reserved_i;        /* table entries; zero */
    const double* sigma;           /* n cross-sections, m^2 */
    double   reserved[4];          /* zero */
} fpic_fusion_spec;
typedef struct fpic_fusion_result {
    uint64_t applications, pairs, below, above, cells, overfull_cells, overfull_particles, yield_hi, yield_lo;
    int32_t  unit_exponent, reserved;
} fpic_fusion_result;
int fpic_fusion(fpic_handle* h, const fpic_fusion_spec* spec, fpic_fusion_result* out, int64_t* grid);
int fpic_fusion_register(fpic_handle* h, const fpic_fusion_spec* spec, int every, int* index);
int fpic_fusion_stats(fpic_handle* h, int index, int scope, fpic_fusion_result* out);
int fpic_fusion_grid(fpic_handle* h, int index, int64_t* grid, int reset);
int fpic_fusion_clear(fpic_handle* h);

/* ---- CART3D fusion product spectra: the yield of a fpic_fusion request (spec.tally) distributed over an energy axis, summed
 * over all pairs of the box — the laboratory energy of one reaction product as a detector would see it (FPIC_FSPEC_PRODUCT:
 * its width is the ion-temperature diagnostic, its shift along a line of sight separates beam-target from thermonuclear
 * yield) or the reacting centre-of-mass energy (FPIC_FSPEC_CM: where the Gamow peak sits).  It is a tally and writes nothing
 * to any particle.  The cells, the key (tag 0xF0510), the order, the pairs, the table and the integer q of every pair are
 * those of fpic_fusion above, so THE WORDS ADD TO THE TALLY: the sum of all bins plus `under` plus `over` equals the yield
 * fpic_fusion reports for spec.tally at the same epoch, as integers, and pairs, below, above, cells, overfull_cells,
 * overfull_particles and unit_exponent are equal as well.  All arithmetic is double, every operation one of + - x / sqrt and
 * rounded once; non-relativistic kinematics.
 *   host numbers   m_a, m_b the species' masses, m3 = product_mass, m4 = other_mass: M = m_a + m_b; f_a = m_a / M,
 *              f_b = m_b / M; m_ab = (m_a m_b) / M; cc = c c, c = 2.998e8; hk = (0.5 m_ab) cc; kf = ((2 m4) / (m3 (m3 + m4))) / cc;
 *              h3 = (0.5 m3) cc; inv_w = bins / (hi - lo); a line of sight n = los / sqrt((lx lx + ly ly) + lz lz).
 *   one pair   inside the table, owner o, partner p, g as in fpic_fusion: K = hk (g g).  Axis CM: x = K.  Axis PRODUCT:
 *              Et = q_value + K, held to 0 from below; u3 = sqrt(Et kf); V_i = (f_o v_o,i) + (f_p v_p,i) with f_o the mass
 *              fraction of the owner's species; w_i = V_i + (u3 n_i); x = h3 ((w_x w_x + w_y w_y) + w_z w_z).
 *   isotropic  los all zero: n is drawn exactly, with no trigonometry, from the blocks Philox4x32-10(counter (id_o, epoch,
 *              stream, 0xF0520 + 16 [the owner is of species_b and a != b] + a), key seed), a = 0 .. 7, two tries each, (w0, w1)
 *              then (w2, w3): x1 = ((w + 0.5) 2^-31) - 1, x2 likewise, s = x1 x1 + x2 x2; the first try with s < 1 gives
 *              r = sqrt(1 - s), n = ((2 x1) r, (2 x2) r, 1 - (2 s)); after sixteen rejections (probability 2e-11) n = (0, 0, 1).
 *   binning    x < lo adds q to `under`, !(x < hi) to `over`; otherwise bin min((int)((x - lo) inv_w), bins - 1) gets q.
 *   the words  words[bins + 2][2]: entry k < bins is bin k, entry bins is `under`, entry bins + 1 is `over`; an entry is
 *              (hi, lo) with lo < 2^32 and stands for hi 2^32 + lo in units of 2^unit_exponent reactions.  A registered
 *              operator is exact for at least 2^23 applications between two drains (fpic_fusion_spectrum_read with reset);
 *              nothing detects an overflow beyond that.
 * fpic_fusion_spectrum tallies now (synchronous): `out` is what fpic_fusion returns for spec.tally (the yield counts every
 * pair inside the table, inside or outside [lo, hi)), `words` the (bins + 2) x 2 words; either may be NULL.
 * fpic_fusion_spectrum_register copies the table and makes the spectrum run at the end of every sub-step whose number is a
 * multiple of `every`, after the operators of fpic_fusion_register and before the recorders, in registration order, with
 * epoch (uint32)(sub-step + spec.tally.epoch); its words accumulate on the device with no host synchronisation.  At most
 * FPIC_FUSION_SPECTRUM_MAX_OPS operators.  fpic_fusion_spectrum_read copies the totals and the words since registration or
 * the last reset and, with reset != 0, zeroes them and `applications` behind the copy in stream order (out and words may be
 * NULL with reset != 0).  fpic_fusion_spectrum_clear drops every registered spectrum.  Registrations are not part of a
 * checkpoint.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, whatever fpic_fusion refuses of spec.tally, a reserved word that is not zero,
 * an axis that is neither, bins outside 1 .. 256, lo not finite, hi <= lo or not finite, q_value not finite, (axis PRODUCT) a
 * mass not (> 0 and finite), a line of sight that is not finite or whose norm is zero or not finite, every < 1, a fifth
 * registration, an index outside the registered operators, a read with neither out, words nor reset; FPIC_ERR_STATE: a
 * handle that is not CART3D, and a handle with a domain decomposition (as fpic_fusion: a rank cannot pair a cell alone). */
#define FPIC_FUSION_SPECTRUM_MAX_OPS  4
#define FPIC_FUSION_SPECTRUM_BINS_MAX 256
#define FPIC_FSPEC_CM      0
#define FPIC_FSPEC_PRODUCT 1
typedef struct fpic_fusion_spectrum_spec {
    fpic_fusion_spec tally;        /* the pairs and their yields */
    int32_t  axis, bins;           /* FPIC_FSPEC_*; 1 .. FPIC_FUSION_SPECTRUM_BINS_MAX */
    double   lo, hi;               /* J: the axis' range [lo, hi) */
    double   q_value;              /* J: the reaction's energy release, may be negative */
    double   product_mass, other_mass;   /* kg: the product that is binned and the other one (axis PRODUCT) */
    double   los[3];               /* the line of sight; all zero: isotropic emission */
    double   reserved[4];          /* zero */
} fpic_fusion_spectrum_spec;
int fpic_fusion_spectrum(fpic_handle* h, const fpic_fusion_spectrum_spec* spec, fpic_fusion_result* out, uint64_t* words);
int fpic_fusion_spectrum_register(fpic_handle* h, const fpic_fusion_spectrum_spec* spec, int every, int* index);
int fpic_fusion_spectrum_read(fpic_handle* h, int index, fpic_fusion_result* out, uint64_t* words, int reset);
int fpic_fusion_spectrum_clear(fpic_handle* h);

/* ---- CART3D prescribed external forces: a field (V/m) or an acceleration (m/s^2) given in closed form — up to four
 * plane waves over the box, a window, tapers along the axes and an envelope in time — that kicks the stored velocities of
 * one species, as a call or registered to run after every sub-step.  It acts per particle at the particle's own stored
 * position: no grid, no gather, the fields and their diagnostics untouched, and a decomposed box takes it as one handle does.
 * The result depends on the request, s and the particle's own state alone — not on the slot, the binning, the rank or the id;
 * no random number is drawn.  All arithmetic is double, every operation rounded once; p is the stored position in box
 * fractions, v the stored velocity in units of c (under both solvers the half-time velocity, the position at the integer
 * time), T the handle's precision.
 *   numbers    (host, once per application) s = (uint64)(sub-step count + epoch), the count being the handle's own since
 *              create (as fpic_collide_register counts).  kq = (charge dt) / (mass c) for FPIC_FORCE_FIELD,
 *              kq = dt / c for FPIC_FORCE_ACCEL (the same for every species).  lo_f[a] = lo[a] / L_a, hi_f[a] = hi[a] / L_a,
 *              w[a] = hi_f[a] - lo_f[a].  Per wave k: tw = nu_k (double) s, tfrac_k = tw - floor(tw) (nu in turns per
 *              sub-step).  The request is ACTIVE iff start <= s <= stop; an inactive one enqueues nothing and counts no
 *              application.  Envelope table of K intervals (K + 1 nodes, node 0 at s = start, node K at s = stop):
 *              g = ((double)(s - start) K) / (double)(stop - start), j = min((int) g, K - 1), r = g - j,
 *              env = tab[j] + (tab[j+1] - tab[j]) r; without a table env = 1.  scale = kq env.
 *   window     a live particle is inside iff lo_f[a] <= p[a] < hi_f[a] on all three axes (compared in double); one outside
 *              keeps every bit and is not counted.
 *   taper      per axis with a table of K intervals (node 0 at lo, node K at hi): f = (p[a] - lo_f[a]) / w[a], and the
 *              lookup of fpic_load_profile: g = f K, j = min((int) g, K - 1), s = g - j, value = tab[j] + (tab[j+1] -
 *              tab[j]) s.  taper = (tx ty) tz over the tables present (a missing table: no multiply).
 *   waves      theta = (m0 p0 + m1 p1) + m2 p2 (the modes as doubles), arg = (theta - tfrac_k) + phase_k,
 *              c_k = cospi(2 arg) (the device's function, as the loader's); zero mode, nu and phase give exactly 1.
 *   kick       e[a] = amp_0[a] c_0, then e[a] = e[a] + amp_k[a] c_k for k = 1 ..; sc = scale, or scale taper with any taper
 *              table; d[a] = sc e[a]; v'[a] = v[a] + d[a], stored as (T) v'[a].  Every inside particle is stored and
 *              counted as `kicked`, also when d is zero.
 * Positions are never written, so the fields stay valid and fpic_precalc is not needed.  A dead slot of a rank of a
 * decomposition is skipped and not counted.
 * Where the kick sits.  The hook runs after the move, at the new position and the new time.  Without B a kick there equals
 * adding the field to the two half-kicks of the next push: the leapfrog scheme with the total field.  With B the external
 * kick comes wholly before the Boris rotation instead of straddling it; the difference is an operator-splitting term of
 * order (omega_c dt) times the kick.
 * Tallies (exact: the fixed point of the energy diagnostics, units of 2^-80, 128-bit two's complement, low word first).  Per
 * kicked particle work_fixed gains floor(|(T)v'|^2 2^80) - floor(|v|^2 2^80), the squared norms ((x x + y y) + z z) of the
 * stored values in double, and impulse_fixed[a] gains floor((T)v'[a] 2^80) - floor(v[a] 2^80).  work = (0.5 m W c^2) times
 * the double nearest to the sum 2^-80 (J); impulse[a] = (m W c) times the same of its sum (kg m/s).  A term outside the
 * diagnostics' range (|term| >= 2^15, or not finite) adds nothing and makes its double NaN.
 * fpic_force applies the request now, at the current count (synchronous), and returns its tallies (applications 1, or 0 when
 * the request is not active).  fpic_force_register makes it run at the end of every sub-step, directly after the sub-step
 * is counted and before every other registered operator and every recorder — all of them see the kicked state — in
 * registration order; at most FPIC_FORCE_MAX_OPS requests, *index names the request.  The tables are copied at the call.
 * Nothing is synchronised: fpic_force_stats reads the totals since registration (scope as for the diagnostics: GLOBAL with a
 * communicator adds the ranks' integers, whatever the decomposition; applications is the same on every rank and is not
 * summed).  fpic_force_clear drops every request.  Registrations are not part of a checkpoint.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, an unknown kind, a species the handle does not have, nwaves outside 1 ..
 * FPIC_FORCE_MAX_WAVES, a value that is not finite (amp, nu, phase, lo, hi, a table's node), a window not within
 * 0 <= lo < hi <= L, |mode| > 2^15, a node count of 1 or above FPIC_FORCE_TABLE_MAX, a null table with a node count,
 * start > stop, an envelope table with stop == start or stop == FPIC_FORCE_FOREVER, a reserved word that is not zero, a
 * ninth registration, an index outside the registered requests; FPIC_ERR_STATE: a handle that is not CART3D. */
#define FPIC_FORCE_FIELD     0
#define FPIC_FORCE_ACCEL     1
#define FPIC_FORCE_MAX_WAVES 4
#define FPIC_FORCE_MAX_OPS   8
#define FPIC_FORCE_TABLE_MAX 1025
#define FPIC_FORCE_FOREVER   (~(uint64_t)0)
typedef struct fpic_force_wave {
    double  amp[3];                /* V/m (FIELD) or m/s^2 (ACCEL) */
    int32_t mode[3];               /* whole periods over the box per axis, |m| <= 2^15 */
    int32_t reserved;              /* zero */
    double  nu, phase;             /* turns per sub-step; turns */
} fpic_force_wave;
typedef struct fpic_force_spec {
    int32_t  species, kind;        /* FPIC_FORCE_FIELD 0, _ACCEL 1 */
    int32_t  nwaves, reserved_i32; /* 1 .. FPIC_FORCE_MAX_WAVES; zero */
    uint64_t epoch, start, stop;   /* s = sub-step count + epoch; active for start <= s <= stop (FPIC_FORCE_FOREVER: no end) */
    double   lo[3], hi[3];         /* the window, metres: 0 <= lo < hi <= L (the whole box: 0 and L) */
    fpic_force_wave wave[FPIC_FORCE_MAX_WAVES];
    uint32_t taper_n[3], envelope_n;   /* nodes; 0 = no table */
    const double* taper[3];
    const double* envelope;
    double   reserved[4];          /* zero */
} fpic_force_spec;
typedef struct fpic_force_result {
    uint64_t applications, kicked;
    uint64_t work_fixed[2];        /* low word, high word */
    uint64_t impulse_fixed[3][2];
    double   work, impulse[3];     /* J; kg m/s */
} fpic_force_result;
int fpic_force(fpic_handle* h, const fpic_force_spec* spec, fpic_force_result* out);
int fpic_force_register(fpic_handle* h, const fpic_force_spec* spec, int* index);
int fpic_force_stats(fpic_handle* h, int index, int scope, fpic_force_result* out);
int fpic_force_clear(fpic_handle* h);

/* ---- CART3D windowed background collisions with a tabulated cross-section: the Monte Carlo operator of fpic_collide
 * against a background gas that occupies a WINDOW of the box with a separable density profile, whose cross-section is a
 * table over the relative speed, and whose exchange of momentum and energy with the species is tallied exactly — a gas puff,
 * a neutral-beam target, a cold edge layer, a beam dump.  EXCHANGE and ELASTIC as fpic_collide has them; there is no RELAX.
 * It acts per particle at the particle's own stored position, so a decomposed box takes it as one handle does.  What
 * happens to particle i (the id the box carries) depends on the request, the epoch, i and its stored state alone — not on
 * the slot, the binning or the rank.  All arithmetic is double, every operation rounded once; p is the stored position in
 * box fractions, v the stored velocity in units of c, T the handle's precision.
 *   words      W(b) = Philox4x32-10(counter (i, epoch, stream, 0x6A500 + b), key (seed_lo, seed_hi)): a tag of its own
 *              (fpic_load 0x10AD, fpic_collide 0xC0110/1, fpic_pair 0xC0120.., fpic_fusion 0xF0510), so a gas operator
 *              never correlates with another operator on the same seed.  W(0) = (w0, w1, w2, w3): candidate, acceptance,
 *              two direction words; W(1): the partner's three normals n[a] (the loader's Box-Muller step).
 *   numbers    (host, once per application) column = (density c) tau with c = 2.998e8 (m^-2: sigma column is a number);
 *              dg = (g_hi - g_lo) / (n - 1), inv_dg = (n - 1) / (g_hi - g_lo); per interval k = 0 .. n - 2
 *              b_k = max(S[k], S[k+1]) g_{k+1} with g_{k+1} = g_lo + (k+1) dg, the last interval with g_hi;
 *              x_max = column max_k b_k — the interval-wise bound, not max(S) g_hi: a resonance does not pay for its peak
 *              at every speed; P_max = -expm1(-x_max); K = (uint64) ldexp(P_max, 32); M = mass_ratio / (1 + mass_ratio),
 *              1 for +inf; lo_f[a] = lo[a] / L_a, hi_f[a] = hi[a] / L_a, w[a] = hi_f[a] - lo_f[a].
 *   candidate  a live particle with lo_f[a] <= p[a] < hi_f[a] on all three axes (fpic_force's window, compared in
 *              double) and (uint64) w0 < K: integers and stored values, so candidacy never depends on rounding.  It is a
 *              SET: which of the two tests a pass makes first is its own choice.
 *   partner    vb[a] = drift[a] + vth[a] n[a]; d[a] = v[a] - vb[a]; g = sqrt((d0 d0 + d1 d1) + d2 d2) (fpic_collide's).
 *   table      g < g_lo: counted `below`; g >= g_hi (or NaN): counted `above`; neither collides.  Else fpic_fusion's
 *              lookup: t = (g - g_lo) inv_dg, k = min((int) t, n - 2), sigma = S[k] + (t - k) (S[k+1] - S[k]), then
 *              sigma = min(sigma, max S).
 *   acceptance rho = (tx ty) tz over the taper tables present, fpic_force's taper rule (f = (p[a] - lo_f[a]) / w[a],
 *              g' = f K, j = min((int) g', K - 1), s = g' - j, tab[j] + (tab[j+1] - tab[j]) s); x = ((column rho) sigma) g,
 *              without any taper table x = (column sigma) g; x = min(x, x_max); u = (w1 + 0.5) 2^-32; the candidate
 *              collides iff u x_max < x.  This is the linearised null-collision acceptance of fpic_collide: a candidate
 *              is accepted with x / x_max, not with (1 - exp(-x)) / P_max — exact where x_max << 1.  The nodes of a taper
 *              lie in [0, 1] so that rho <= 1 and the bound holds; the hold to x_max guards the last roundings.
 *   EXCHANGE   v' = vb.
 *   ELASTIC    c = 1 - 2 (w2 + 0.5) 2^-32, s = sqrt(1 - c c), phi = w3 2^-32, nhat = (s cospi(2 phi), s sinpi(2 phi), c);
 *              t = g nhat[a]; r = d[a] - t; q = M r; v'[a] = v[a] - q (fpic_collide's, operation for operation).
 * A particle that does not collide keeps every bit; positions are never written; a dead slot of a rank of a decomposition
 * is never counted.
 * Tallies (exact: the fixed point of fpic_force and the energy diagnostics, units of 2^-80, 128-bit two's complement, low
 * word first).  Per collided particle energy_fixed gains floor(|(T)v'|^2 2^80) - floor(|v|^2 2^80), the squared norms
 * ((x x + y y) + z z) of the stored values in double, and momentum_fixed[a] gains floor((T)v'[a] 2^80) - floor(v[a] 2^80):
 * the SPECIES' gains; the reservoir takes the negatives.  energy = (0.5 m W c^2) times the double nearest to the sum 2^-80
 * (J), momentum[a] = (m W c) times the same of its sum (kg m/s).  A term outside the diagnostics' range (|term| >= 2^15, or
 * not finite) adds nothing and makes its double NaN.
 * fpic_gas applies the request now (synchronous) and returns its result (applications 1); K = 0 — a zero density, an
 * all-zero table — launches nothing and returns zeros, as fpic_collide does.fpic_gas_register makes it run at the end of every sub-step with
 * substep % every == 0, after the operators of fpic_collide_register and before those of fpic_pair_register, in
 * registration order, with epoch (uint32)(substep + spec.epoch); at most FPIC_GAS_MAX_OPS operators, *index names the
 * operator.  The tables are copied at the call.  Nothing is synchronised: fpic_gas_stats reads the totals since
 * registration (GLOBAL with a communicator adds the ranks' integers; applications is the same on every rank and is not
 * summed).  fpic_gas_clear drops every operator (those of fpic_collide_register stay).  Registrations are not part of a
 * checkpoint.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, an unknown kind, a species the handle does not have, a reserved word that
 * is not zero, a density that is negative or not finite, a tau that is not positive and finite, n outside 2 ..
 * FPIC_GAS_TABLE_MAX, a null table, g_lo negative or not finite, g_hi not above g_lo or not finite, a cross-section that
 * is negative or not finite, a drift or vth that is not finite, a negative vth, a mass_ratio that is not positive for
 * ELASTIC or not 0 for EXCHANGE, a window not within 0 <= lo < hi <= L, a taper node count of 1 or above
 * FPIC_GAS_TAPER_MAX, a null taper with a node count, a taper node outside [0, 1], an x_max that is not finite, every
 * below 1, a ninth registration, an index outside the registered operators; FPIC_ERR_STATE: a handle that is not CART3D. */
#define FPIC_GAS_EXCHANGE  0
#define FPIC_GAS_ELASTIC   1
#define FPIC_GAS_MAX_OPS   8
#define FPIC_GAS_TABLE_MAX 4096
#define FPIC_GAS_TAPER_MAX 1025
typedef struct fpic_gas_spec {
    int32_t  species, kind;        /* FPIC_GAS_EXCHANGE 0, _ELASTIC 1 */
    uint64_t seed;
    uint32_t stream, epoch;
    double   density;              /* m^-3: the peak density of the background, >= 0 and finite */
    double   tau;                  /* s: the time one application stands for, > 0 and finite */
    double   g_lo, g_hi;           /* units of c: the table's first and last relative speed */
    int32_t  n, reserved_i;        /* table entries, 2 .. FPIC_GAS_TABLE_MAX; zero */
    const double* sigma;           /* n cross-sections, m^2 */
    double   drift[3], vth[3];     /* the background, units of c; vth >= 0 */
    double   mass_ratio;           /* m_background / m_species > 0, +inf allowed; ELASTIC only, else 0 */
    double   lo[3], hi[3];         /* the window, metres: 0 <= lo < hi <= L (the whole box: 0 and L) */
    uint32_t taper_n[3], reserved_u;   /* nodes, 0 = no table, else 2 .. FPIC_GAS_TAPER_MAX; zero */
    const double* taper[3];        /* the density over the window as a fraction of `density`: nodes in [0, 1] */
    double   reserved[4];          /* zero */
} fpic_gas_spec;
typedef struct fpic_gas_result {
    uint64_t applications, candidates, collided, below, above;
    uint64_t energy_fixed[2];      /* low word, high word */
    uint64_t momentum_fixed[3][2];
    double   energy, momentum[3];  /* J; kg m/s: the species' gains */
} fpic_gas_result;
int fpic_gas(fpic_handle* h, const fpic_gas_spec* spec, fpic_gas_result* out);
int fpic_gas_register(fpic_handle* h, const fpic_gas_spec* spec, int every, int* index);
int fpic_gas_stats(fpic_handle* h, int index, int scope, fpic_gas_result* out);
int fpic_gas_clear(fpic_handle* h);

/* ---- CART3D absorbing particle sinks: the particles of ONE species that a predicate over x y z vx vy vz |v|^2 names are
 * taken out of the species on the device, and what left is accounted for exactly — a wall, a limiter or divertor plate, a
 * beam dump, a loss cone, an evaporative cut of the tail, an absorbing edge layer.  Undecomposed handles only.
 *   predicate  species, nterms, axis, lo, hi, id_mod, id_rem are fpic_select_spec's, with its meaning: a live particle
 *              MATCHES iff fpic_select would select it — every term compared in double, a NaN matches nothing, then the id
 *              rule.  flags = 0: the matching particles are removed.  FPIC_REMOVE_OUTSIDE: the live particles that pass
 *              the id rule and do NOT match every term are removed (the intervals are ANDed, an absorbing edge is the
 *              complement of a brick: "keep the interior" is this flag).  nterms = 0 removes every particle the id rule
 *              passes; with the flag it removes nothing.
 *   survivors  keep every bit of their state and their id.  After the call the species holds n' = n - removed particles in
 *              slots [0, n'), in the slot order they had before (stable): the state after is a function of the state
 *              before, not of any atomic's order.
 *   result     applications; scanned (the live particles before each application, summed); removed; energy_fixed,
 *              momentum_fixed[a]: exact sums in the fixed point of the energy diagnostics (units of 2^-80, 128-bit two's
 *              complement, low word first) of floor(|v|^2 2^80) and floor(v[a] 2^80) over the removed particles, from the
 *              stored velocity, the squared norm ((x x + y y) + z z) in double — what the species LOST; a term >= 2^15 in
 *              magnitude or not finite adds nothing and makes its double NaN (fpic_energy's rule).  energy = (0.5 m W
 *              c^2) times the double nearest to the sum 2^-80 (J), momentum[a] = (m W c) times the same (kg m/s), charge =
 *              removed x the species' charge x macro_weight in double (C).
 * fpic_remove applies the request now (synchronous, as fpic_gas) and returns its result (applications 1).
 * fpic_remove_register makes it run at the end of every sub-step with substep % every == 0, after the fusion spectra and
 * before the recorders: the tallies of that sub-step see the particles that are about to leave, the recorded rows see the
 * thinned box.  Operators run in registration order, at most FPIC_REMOVE_MAX_OPS of them; *index names the operator.
 * UNLIKE the other registered operators a due application reads one 8-byte total back to the host and waits for it: the
 * host has to learn the new particle count.  fpic_remove_stats reads the totals since registration (scope: LOCAL or
 * GLOBAL, the same on an undecomposed handle).  fpic_remove_clear drops every registered operator.  Registrations are not
 * part of a checkpoint.
 * What a removal leaves.  One that took nothing changes nothing: no buffer is swapped, no field or bin table touched.  One
 * that took a particle leaves the species as an upload leaves one (the next sub-step re-bins), and marks it THINNED: its
 * ids are no longer 0 .. n-1, they lie below the species' id span (one past the largest id it was ever given, which does
 * not shrink).  Electrostatic solver (poisson_fft): if the fields were ready the call itself deposits the survivors'
 * charge and solves, so E is the field of the survivors; fields that were not ready stay so.  Full EM (yee): E, B and the
 * readiness are left untouched — the charge of a removed particle stays in the lattice E as a static source, as the
 * surface charge of an absorbing wall does; Gauss's law is not re-imposed.
 * Everything that works per particle or by id keeps working on a thinned species (the push, deposits, fpic_sort, energy,
 * histograms, moments, modes, fpic_select — the way to read a thinned species back —, the series, whose row of a removed
 * tracer is zeros and whose tracer ids are bounded by the id span, fpic_collide, fpic_gas, fpic_force, fpic_pair,
 * fpic_fusion, fpic_fusion_spectrum).  Everything that addresses particles in the caller's order is refused on a thinned
 * species with FPIC_ERR_STATE: fpic_get_particles_of / _range, fpic_get_cells_of / _range, fpic_set_particles_of / _range,
 * fpic_load*, fpic_save_checkpoint, fpic_domain_init.
 * fpic_renumber gives every survivor the id "number of live ids below mine" (on the device: a bitmap over the id span and
 * a popcount scan), clears the mark and sets the id span to n; *n receives n.  Positions, velocities and fields do not
 * change.  After it the caller-order calls and the checkpoint work again on the n survivors, in ascending old id.  A no-op
 * that returns n on a species that is not thinned.  Synchronous.  Refused (FPIC_ERR_STATE) while a series recording or a
 * registered operator of any kind exists on the handle: both name ids or draw per-id random words, which would silently
 * change meaning.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, everything fpic_select refuses of a request (nterms outside 0 .. 7, an axis
 * code outside 0 .. 6, the same axis twice, a NaN bound or not lo < hi, entries past nterms that are not zero, id_rem >=
 * id_mod when id_mod > 1, a species the handle does not have), an unknown flag, a reserved word that is not zero, every
 * below 1, a ninth registration, an index outside the registered operators, a null out of fpic_remove_stats;
 * FPIC_ERR_STATE: a handle that is not CART3D; a decomposed handle (all five calls: a rank's dead slots and its migration
 * tail would need a protocol of their own). */
#define FPIC_REMOVE_OUTSIDE  1u
#define FPIC_REMOVE_MAX_OPS  8
typedef struct fpic_remove_spec {
    int32_t  species, nterms;   /* as fpic_select_spec */
    int32_t  axis[8];
    double   lo[8], hi[8];
    uint32_t id_mod, id_rem;
    uint32_t flags, reserved_u; /* FPIC_REMOVE_OUTSIDE or 0; zero */
    double   reserved[4];       /* zero */
} fpic_remove_spec;
typedef struct fpic_remove_result {
    uint64_t applications, scanned, removed;
    uint64_t energy_fixed[2];      /* low word, high word */
    uint64_t momentum_fixed[3][2];
    double   energy, momentum[3];  /* J; kg m/s: what the species lost */
    double   charge;               /* C */
} fpic_remove_result;
int fpic_remove(fpic_handle* h, const fpic_remove_spec* spec, fpic_remove_result* out);
int fpic_remove_register(fpic_handle* h, const fpic_remove_spec* spec, int every, int* index);
int fpic_remove_stats(fpic_handle* h, int index, int scope, fpic_remove_result* out);
int fpic_remove_clear(fpic_handle* h);
int fpic_renumber(fpic_handle* h, int species, uint64_t* n);

/* ---- CART3D particle sources: ONE species of an undecomposed handle gains particles that are generated on the device by
 * the loader's counter-based rule — a beam into a target plasma, an emitting wall or electrode, the refilling bulk of a
 * sheath, an ionisation source against a limiter, a pellet or a gas puff.  The counterpart of fpic_remove.
 * Capacity.  fpic_reserve raises the capacity of a species (the particles its arrays hold; it starts as the count given to
 * fpic_create / fpic_add_species) to at least `capacity` and reports the capacity it has now; a smaller request changes
 * nothing.  Every particle keeps its bits, its id and its slot, the fields and their readiness stay; the species is left
 * as an upload leaves one (the next sub-step bins it again).  Synchronous; the old arrays are freed.  Operators registered
 * before the call keep running: the cell index that fpic_pair_register, fpic_fusion_register and
 * fpic_fusion_spectrum_register size from the species follows the new capacity here.  Refused
 * (FPIC_ERR_INVALID_ARG): a capacity whose ids would not fit in 32 bits (2^32 - 4096 and above, fpic_add_species's bound).
 * fpic_population reads n (the live particles), the capacity and the id span (one past the largest id the species can
 * hold: n unless fpic_remove has thinned it) of a species on the host; any of the three pointers may be null.  It also
 * works on a rank of a decomposition, where it reports the rank's numbers.  A registered source changes n behind the
 * caller's back: this is how a host learns it.
 * The request.  fpic_inject_spec embeds a fpic_load_spec: species, seed, stream, lo, hi, drift, vth, mode, xamp, xphase,
 * vamp, vphase and the flags LATTICE and PAIRED mean what they mean to fpic_load, and the embedded request passes
 * fpic_load's own checks.  FPIC_LOAD_POS | FPIC_LOAD_VEL are both required, FPIC_LOAD_APPEND is refused, count must be
 * given (~0 is refused).  load.count = the particles per application, load.first = the SEQUENCE NUMBER of the first
 * particle of application 0.  Application k (k = epoch + the applications this registration has made; fpic_inject itself
 * is application `epoch`) generates the sequence numbers j = first + k count + l, l < count.  j is the loader's index i:
 * the first Philox counter word and the lattice index.  A host that resumes a run registers again with epoch = the
 * applications made so far.  Every application keeps fpic_load's bound on 32-bit indices, first_k + count <= 2^32 - 1: application
 * 0 that breaks it is refused with the request, a later one returns FPIC_ERR_STATE.
 * Ids and slots.  Particle l of an application takes the id (id span) + l and the slot n + l of the live set; n and — on a
 * thinned species — the id span grow by count.  A species that is not thinned stays not thinned, ids 0 .. n-1: the
 * caller-order calls and the checkpoint keep working on the grown species.  An application that does not fit
 * (n + count > capacity, or id span + count > 2^32 - 1) changes nothing: fpic_inject returns FPIC_ERR_INVALID_ARG (call
 * fpic_reserve first), a registered application makes the step return FPIC_ERR_STATE.
 * All arithmetic below is double, every operation rounded once; an fp32 handle stores the float rounding.
 *   kind = FPIC_INJECT_VOLUME   position and velocity of sequence number j are EXACTLY fpic_load's for i = j (see there:
 *              words, fractions, position with its displacement and wrap, Box-Muller velocity, PAIRED): uniform in the
 *              window [lo, hi) or on the Kronecker lattice, a drifting Maxwellian.  fpic_inject(first = N, count = m)
 *              into a species of N equals fpic_load(first = N, count = m) into a species of N + m, bit for bit.  Two
 *              species fed the same seed, stream and sequence coincide exactly: an electron-ion source creates no net
 *              charge.  axis, side and plane must be zero.
 *   kind = FPIC_INJECT_FLUX     emission through the plane x[axis] = plane (metres) towards side = +1 or -1, the
 *              flux-weighted half-Maxwellian of thermal speed vth[axis].  With t1 < t2 the two other axes:
 *              words      W(0) = (w0, w1, w2, .) and W(1) = (u0, u1, u2, u3) as fpic_load (or the lattice words for W(0))
 *              tangential p_t = lo[t]/L_t + (w_t 2^-32) (hi[t] - lo[t])/L_t for t = t1, t2 (one multiply, one add)
 *              time       f_t = w_axis 2^-32: the fraction of the step the particle has already flown
 *              normals    n0 = sqrt(-2 ln((u0 + 0.5) 2^-32)) cospi(2 u1 2^-32), n1 = the same radius times
 *                         sinpi(2 u1 2^-32) (fpic_load's n0, n1); s = sqrt(-2 ln((u2 + 0.5) 2^-32)), a Rayleigh deviate
 *                         (fpic_load's radius of n2), 0 < s <= 6.76
 *              velocity   v_t1 = drift[t1] + vth[t1] n0, v_t2 = drift[t2] + vth[t2] n1 (one multiply, one add each),
 *                         v_axis = side (vth[axis] s)
 *              normal     p_axis = plane/L_axis + (v_axis (dt c / L_axis)) f_t (two multiplies, one add), dt the handle's
 *                         step and c = 2.998e8 as the push has them; stored cast and wrapped into [0, 1) as every position
 *              lo[axis], hi[axis] must be a valid interval and are not used.  Refused for FLUX: an axis outside 0 .. 2, a
 *              side that is not +1 or -1, a plane outside [0, L_axis] or not finite, drift[axis] != 0, PAIRED, any
 *              non-zero xamp, vamp or mode.
 * The result: applications; injected; energy_fixed, momentum_fixed[a]: exact sums in the fixed point of the energy
 * diagnostics (units of 2^-80, 128-bit two's complement, low word first) of floor(|v|^2 2^80) and floor(v[a] 2^80) over the
 * new particles, from the STORED velocity (after the rounding to the handle's precision), by fpic_energy's rule (a term >=
 * 2^15 in magnitude or not finite adds nothing and makes its double NaN) — what the species GAINED: fpic_energy_now after
 * the call minus before it, word for word.  energy, momentum[a] and charge = injected x the species' charge x macro_weight
 * as fpic_remove_result has them.
 * fpic_inject applies the request now (synchronous) and returns its result (applications 1).  fpic_inject_register makes
 * it run at the end of every sub-step with substep % every == 0, after the registered sinks and before the recorders: a
 * sink registered beside a source leaves that sub-step's fresh particles alive, and the recorded rows count them.
 * Sources run in registration order, at most FPIC_INJECT_MAX_OPS of them; *index names the source.  No count is read back:
 * the host knows n + count in advance.  fpic_inject_stats reads the totals since registration (scope: LOCAL or GLOBAL, the
 * same on an undecomposed handle), fpic_inject_clear drops every registered source.  Registrations are not part of a
 * checkpoint.  count = 0 and an application that is not due change nothing and launch nothing.
 * What an application leaves: n raised, the species as an upload leaves one (nothing binned, no census: the next sub-step
 * bins the WHOLE species again).  Electrostatic solver (poisson_fft): if the fields were ready the call itself deposits the
 * grown population and solves, so the next sub-step gathers its field; fields that were not ready stay so.  Full EM (yee):
 * E, B and the readiness stay — a charge that appears without a current is a static source in the lattice E, Gauss's law
 * is not re-imposed; inject a neutral pair of species on one seed, stream and sequence instead.
 * A checkpoint of a grown, unthinned species is saved as any other and restores into a handle whose species has the
 * capacity (fpic_reserve first): the restored count is the file's.
 * fpic_renumber is refused while a source is registered, as for every registered operator.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, what fpic_load refuses of the embedded request, the flag and count rules
 * above, an unknown kind, the FLUX rules above, VOLUME with a non-zero axis, side or plane, a reserved word that is not
 * zero, every below 1, a ninth registration, an index outside the registered sources, a null out of fpic_inject_stats;
 * FPIC_ERR_STATE: a handle that is not CART3D; a decomposed handle (fpic_reserve and the four fpic_inject calls: a rank's
 * arrivals ride on its next push and its message buffers were sized from the capacity). */
#define FPIC_INJECT_VOLUME   0
#define FPIC_INJECT_FLUX     1
#define FPIC_INJECT_MAX_OPS  8
typedef struct fpic_inject_spec {
    fpic_load_spec load;        /* count: particles per application; first: the sequence number of application 0 */
    int32_t  kind;              /* FPIC_INJECT_VOLUME or FPIC_INJECT_FLUX */
    int32_t  axis, side;        /* FLUX: 0 .. 2; +1 or -1 */
    int32_t  reserved_i;        /* zero */
    double   plane;             /* FLUX: metres, within [0, L_axis] */
    uint64_t epoch;             /* the applications made before this registration (a resumed run) */
    double   reserved[4];       /* zero */
} fpic_inject_spec;
typedef struct fpic_inject_result {
    uint64_t applications, injected;
    uint64_t energy_fixed[2];      /* low word, high word */
    uint64_t momentum_fixed[3][2];
    double   energy, momentum[3];  /* J; kg m/s: what the species gained */
    double   charge;               /* C */
} fpic_inject_result;
int fpic_reserve(fpic_handle* h, int species, uint64_t capacity, uint64_t* capacity_out);
int fpic_population(fpic_handle* h, int species, uint64_t* n, uint64_t* capacity, uint64_t* id_span);
int fpic_inject(fpic_handle* h, const fpic_inject_spec* spec, fpic_inject_result* out);
int fpic_inject_register(fpic_handle* h, const fpic_inject_spec* spec, int every, int* index);
int fpic_inject_stats(fpic_handle* h, int index, int scope, fpic_inject_result* out);
int fpic_inject_clear(fpic_handle* h);

/* ---- CART3D electron-impact ionisation of a background gas: a projectile species (the electrons) collides with the gas of
 * fpic_gas — a window of the box, a separable density profile, a cross-section tabulated over the relative speed — and every
 * collision is an EVENT that leaves a new electron and a new ion behind, on the device: a gas puff, a breakdown, a beam that
 * strikes a neutral target, a cold edge layer.  A source and a sink's bookkeeping coupled per event; undecomposed handles
 * only.  What happens to projectile i (the id the box carries) depends on the request, the epoch, the ids and the stored
 * state alone — not on the slots, the binning or the order any atomic took.  All arithmetic is double, every operation
 * rounded once; p is the stored position in box fractions, v the stored velocity in units of c, T the handle's precision.
 *   request    species (the projectile), seed, stream, epoch, density, tau, g_lo, g_hi, n, sigma, drift, vth, lo, hi, taper_n,
 *              taper mean what they mean to fpic_gas (there is no kind and no mass_ratio).  electron: the species that
 *              receives the secondary, which may be the projectile species itself; ion: the species that receives the ion,
 *              different from both; g_threshold (units of c): g_threshold^2 = 2 E_ion / (m c^2) of the projectile, >= 0 and
 *              finite, and g_lo >= g_threshold: the table starts at or above the threshold, so an event always has energy
 *              to share.
 *   words      W(b) = Philox4x32-10(counter (i, epoch, stream, 0x1051E0 + b), key (seed_lo, seed_hi)): a tag of its own
 *              beside 0x10AD, 0xC0110/1, 0xC0120.., 0xF0510 and 0x6A500.  W(0) = (w0, w1, w2, w3): candidate, acceptance,
 *              the two direction words of the primary; W(1): the partner's normals; W(2) = (r0, r1, r2, .): the energy
 *              share and the two direction words of the secondary (the fourth word is unused).
 *   candidate, partner, table, acceptance   fpic_gas's, operation for operation, on these words: the window and (uint64) w0 <
 *              K; vb[a] = drift[a] + vth[a] n[a], d = v - vb, g = sqrt((d0 d0 + d1 d1) + d2 d2); g < g_lo counted `below`,
 *              g >= g_hi (or NaN) `above`; the lookup with its hold, the tapers, x = min(((column rho) sigma) g, x_max), u =
 *              (w1 + 0.5) 2^-32; an EVENT iff u x_max < x.
 *   outcome    gp2 = g g - g_threshold g_threshold; r = (r0 + 0.5) 2^-32; a1 = r gp2; a2 = gp2 - a1; g1 = sqrt(a1), g2 =
 *              sqrt(a2); n1 = fpic_gas ELASTIC's nhat on (w2, w3), n2 the same formula on (r1, r2);
 *              primary v'[a] = vb[a] + g1 n1[a]; secondary vs[a] = vb[a] + g2 n2[a]; ion vi[a] = vb[a].
 *              The gas atom is heavy: it keeps its velocity, and the two electrons share g^2 - g_threshold^2 in its frame,
 *              isotropically and with a uniform share.  The RECOIL of the ion IS NEGLECTED (momentum is not conserved by
 *              m_e / m_i of the electrons' change; the tallies below say exactly what each species gained).  Each velocity is
 *              cast to T when stored.  The secondary and the ion take the primary's stored position, bit for bit.  A
 *              projectile without an event keeps every bit; positions of existing particles are never written.
 *   placement  the events of one application in ascending id of their primary: event number l gives the electron in slot
 *              n_e + l with id (id span of `electron`) + l, and the ion in slot n_i + l with id (id span of `ion`) + l, n
 *              and the id spans those before the application.  With electron == species only the old [0, n) is scanned.  A
 *              species that is not thinned stays not thinned; a thinned one stays thinned and its id span grows
 *              (fpic_inject's rule).
 *   fit        with M events: n + M beyond either target's capacity, or an id span beyond 2^32 - 1, refuses the
 *              application and NOTHING has changed — no velocity, no slot, no tally: fpic_ionize returns
 *              FPIC_ERR_INVALID_ARG (call fpic_reserve first), a registered application makes the step return FPIC_ERR_STATE.
 * The result: applications, candidates, below, above, ionised (= M); primary: the projectile species' gains, fpic_gas's
 * before/after terms of the stored velocities of the primaries; electron, ion: what each target gained, fpic_inject's terms
 * of the STORED velocities of the new particles, and charge = ionised x the species' charge x macro_weight (primary.charge
 * is 0).  Sums are exact, in the fixed point of the energy diagnostics (units of 2^-80, 128-bit two's complement, low word
 * first); a term outside its range adds nothing and makes its double NaN.
 * fpic_ionize applies the request now (synchronous) and settles itself; K = 0 launches nothing and returns zeros.
 * fpic_ionize_register makes it run at the end of every sub-step with substep % every == 0, after
 * the sources, before the burners: a beam injected on a sub-step can ionise on it, and the recorded rows count the new
 * particles —, in registration order, with epoch (uint32)(substep + spec.epoch); at most FPIC_IONIZE_MAX_OPS ionisers.  The
 * tables are copied at the call.  A due application reads ONE 8-byte count back (the events: the host has to learn the new
 * n) and is counted once it has succeeded.  fpic_ionize_stats reads the totals since registration, fpic_ionize_clear drops
 * every ioniser (other operators stay).  Registrations are not part of a checkpoint; fpic_renumber is refused while one exists.
 * What an application leaves.  M = 0: nothing changes, nothing is re-binned.  Else the projectile species has new velocities
 * only and keeps its binning (unless it is also the electron target); each target is as fpic_inject leaves one (n raised,
 * nothing binned: the next sub-step bins the whole species).  Electrostatic solver with ready fields: the call — or the
 * hook, once per sub-step after the last ioniser due — deposits and solves again.  Full EM: E, B and the readiness stay; an
 * electron and an ion of opposite charge at one position add no net charge.
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, everything fpic_gas refuses of the shared fields, an electron or ion the
 * handle does not have, ion equal to species or electron, a g_threshold that is negative or not finite, g_lo < g_threshold,
 * a reserved word that is not zero, every below 1, a ninth registration, an index outside the registered ionisers, a null
 * out of fpic_ionize_stats; FPIC_ERR_STATE: a handle that is not CART3D; a decomposed handle (all four calls). */
#define FPIC_IONIZE_MAX_OPS 8
typedef struct fpic_ionize_spec {
    int32_t  species, electron;    /* the projectile; the species that receives the secondary (may equal species) */
    int32_t  ion, reserved_i;      /* the species that receives the ion (differs from both); zero */
    uint64_t seed;
    uint32_t stream, epoch;
    double   density;              /* m^-3, as fpic_gas_spec */
    double   tau;                  /* s */
    double   g_lo, g_hi;           /* units of c; g_lo >= g_threshold */
    double   g_threshold;          /* units of c: sqrt(2 E_ion / (m c^2)) of the projectile; >= 0 and finite */
    int32_t  n, reserved_n;        /* table entries, 2 .. FPIC_GAS_TABLE_MAX; zero */
    const double* sigma;           /* n ionisation cross-sections, m^2 */
    double   drift[3], vth[3];     /* the gas, units of c; vth >= 0 */
    double   lo[3], hi[3];         /* the window, metres */
    uint32_t taper_n[3], reserved_u;   /* nodes, 0 = no table, else 2 .. FPIC_GAS_TAPER_MAX; zero */
    const double* taper[3];
    double   reserved[4];          /* zero */
} fpic_ionize_spec;
typedef struct fpic_ionize_gain {
    uint64_t energy_fixed[2];      /* low word, high word */
    uint64_t momentum_fixed[3][2];
    double   energy, momentum[3];  /* J; kg m/s: what the species gained */
    double   charge;               /* C */
} fpic_ionize_gain;
typedef struct fpic_ionize_result {
    uint64_t applications, candidates, below, above, ionised;
    fpic_ionize_gain primary, electron, ion;
} fpic_ionize_result;
int fpic_ionize(fpic_handle* h, const fpic_ionize_spec* spec, fpic_ionize_result* out);
int fpic_ionize_register(fpic_handle* h, const fpic_ionize_spec* spec, int every, int* index);
int fpic_ionize_stats(fpic_handle* h, int index, int scope, fpic_ionize_result* out);
int fpic_ionize_clear(fpic_handle* h);

/* ---- CART3D fusion burn: the pairs of fpic_fusion REACT — a macro-particle of species_a and one of species_b leave their
 * species, and one new particle of product_a and one of product_b are born, on the device: burn-up, alpha heating, a
 * fast-ion tail.  The handle has one macro_weight W for all species, so one macro-reactant of each kind becomes exactly one
 * macro-product of each kind; nothing is weighted.  Undecomposed handles only.  What an application does depends on the
 * request, the epoch, the ids and the stored state alone — not on the slots, the binning or the order any atomic took.  All
 * arithmetic is double, every operation one of + - x / sqrt and rounded once; v is the stored velocity in units of c, T the
 * handle's precision; non-relativistic kinematics, as fpic_fusion_spectrum's.
 *   pairs      the cells, the order inside a cell (ascending (key, id)), the pair sets and N_L are fpic_fusion's: unlike
 *              species the Nm pairs many[j] with few[j mod Nf] (`many` the species with more, a tie: species_a), N_L = Nf;
 *              like species (s[2t], s[2t+1]) with N_L = N, an odd cell (s0,s1), (s1,s2), (s2,s0) with N_L = N / 2 and then
 *              (s[3+2t], s[4+2t]); a cell with more than FPIC_PAIR_CELL_MAX particles of either species is skipped and
 *              counted.  The pair's OWNER is its `many` particle, or s[q] of the place q that fpic_fusion's like_pair names.
 *              The key is word 0 of Philox4x32-10(counter (id, epoch, stream, 0xB0510), key (seed_lo, seed_hi)): a tag of
 *              its own, so a burner never correlates with a tally (0xF0510) or a Coulomb operator (0xC0120) on the same seed.
 *   g, table   u = v_o - v_p, g = sqrt((ux ux + uy uy) + uz uz); g < g_lo counted `below`, g >= g_hi (or NaN) `above`, both
 *              do nothing; else the lookup of fpic_fusion with its hold at max sigma, operation for operation.
 *   probability   y = ((((W W) N_L) tau) / dV) (sigma (g c)), fpic_fusion's yield of the pair before its floor; P = y / W.
 *              The pair is ACCEPTED iff (u + 0.5) 2^-32 < P, u = word 0 of the owner's block Philox4x32-10(counter (id_o,
 *              epoch, stream, 0xB0511 + [the owner is of species_b and a != b]), key seed).  P >= 1 always accepts and is
 *              counted `saturated`.  max sigma = 0 launches nothing.
 *   conflicts  a particle burns at most once.  Unlike species: few[f] is the partner of the many places f, f + Nf, f + 2 Nf,
 *              ...: of the accepted pairs of that chain only the one with the lowest place REACTS, the others are counted
 *              `blocked`.  Like species: the pairs are disjoint but for the triple of an odd cell, where the first accepted
 *              pair in the order (s0,s1), (s1,s2), (s2,s0) reacts.  accepted = burnt + blocked.
 *   outcome    host numbers as fpic_fusion_spectrum's with m3 = the mass of product_a and m4 = the mass of product_b (or
 *              other_mass): M = m_a + m_b, f_a = m_a / M, f_b = m_b / M, hk = (0.5 ((m_a m_b) / M)) (c c),
 *              kf = ((2 m4) / (m3 (m3 + m4))) / (c c), r34 = m3 / m4.  With a the species_a reactant and b the species_b
 *              reactant (like species: owner and partner): K = hk (g g); Et = q_value + K, held to 0 from below;
 *              u3 = sqrt(Et kf); u4 = r34 u3; V_i = (f_a v_a,i) + (f_b v_b,i); n the exact isotropic direction of
 *              fpic_fusion_spectrum (two tries per block, x = ((w + 0.5) 2^-31) - 1, s = x1 x1 + x2 x2 < 1, n = ((2 x1) r,
 *              (2 x2) r, 1 - (2 s)) with r = sqrt(1 - s); after sixteen rejections (0, 0, 1)) on the blocks
 *              Philox4x32-10(counter (id_a, epoch, stream, 0xB0520 + k), key seed), k = 0 .. 7, of the species_a reactant (a
 *              reactant is in one event at most, so every event has blocks of its own); w3_i = V_i + (u3 n_i);
 *              w4_i = V_i - (u4 n_i).  Product 3 takes the stored position of the species_a reactant bit for bit and the
 *              velocity (T) w3; product 4 the position of the species_b reactant and (T) w4.
 *   placement  the events of one application in ascending id of their species_a reactant (like species: of the owner): event
 *              number l puts product 3 in slot n3 + l with id (id span of product_a) + l and product 4 in slot n4 + l with
 *              id (id span of product_b) + l, n and the id spans those before the application (fpic_ionize's rule).
 *   removal    both reactants of every event leave their species exactly as fpic_remove takes a particle out: the survivors
 *              keep every bit, their ids and their order, the species is THINNED (fpic_renumber is refused while a burner
 *              is registered), the handle's n follows the first species.
 *   fit        with M events: n + M beyond a product's capacity, or an id span beyond 2^32 - 1, refuses the application and
 *              NOTHING has changed — no slot, no velocity, no tally, no thinned mark: fpic_burn returns FPIC_ERR_INVALID_ARG
 *              (call fpic_reserve first), a registered application makes the step return FPIC_ERR_STATE.
 * The result: applications; pairs (inside the table), below, above, cells, overfull_cells, overfull_particles as fpic_fusion
 * counts them; accepted, blocked, saturated, burnt (= M).  reactant_a, reactant_b: what the species LOST, fpic_remove's
 * terms of the stored velocities of the particles that left (like species: reactant_a carries both members of every pair
 * and reactant_b is zeros); product_a, product_b: what each GAINED, fpic_inject's terms of the stored velocities of the new
 * particles.  With product_b = -1 the fourth particle leaves the box: nothing is stored, and product_b of the result carries
 * what it took away, from its double velocity w4 with mass other_mass and charge 0 — the books stay closed.  charge = the
 * count x the species' charge x macro_weight.  Sums are exact, in the fixed point of the energy diagnostics (units of 2^-80,
 * 128-bit two's complement, low word first); a term outside its range adds nothing and makes its double NaN.
 * fpic_burn applies the request now (synchronous) and settles itself.  fpic_burn_register makes it run at the end of every
 * sub-step with substep % every == 0, after the ionisers and before the recorders, in registration order, with epoch
 * (uint32)(substep + spec.epoch): a tally registered beside a burner sees the unburnt plasma of that sub-step, the recorded
 * rows the burnt one; at most FPIC_BURN_MAX_OPS burners.  The table is copied at the call.  A due application reads ONE
 * 8-byte count back (the events) and is counted once it has succeeded.  fpic_burn_stats reads the totals since
 * registration, fpic_burn_clear drops every burner (other operators stay).  Registrations are not part of a checkpoint.
 * What an application leaves.  M = 0: nothing changes, nothing is re-binned, no species is thinned.  Else each reactant
 * species is as fpic_remove leaves one and each product as fpic_inject leaves one.  Electrostatic solver with ready fields:
 * the call — or the hook, once per sub-step after the last burner due — deposits and solves again.  Full EM: E, B and the
 * readiness stay; an event moves charge within a cell without a current (the static-source caveat of the sinks and sources).
 * Refused (FPIC_ERR_INVALID_ARG): a null spec, everything fpic_fusion refuses of the shared fields (species_a, species_b,
 * tau, n, sigma, g_lo, g_hi, the yield bound), a product_a the handle does not have, a product_b that is neither -1 nor a
 * species of the handle, a product equal to a reactant or to the other product, other_mass not positive and finite with
 * product_b = -1 or not zero otherwise, a q_value that is not finite, a reserved word that is not zero, every below 1, a
 * fifth registration, an index outside the registered burners, a null out of fpic_burn_stats; FPIC_ERR_STATE: a handle that
 * is not CART3D; a decomposed handle (all four calls). */
#define FPIC_BURN_MAX_OPS 4
typedef struct fpic_burn_spec {
    int32_t  species_a, species_b;     /* the reactants; equal: like species (D-D) */
    int32_t  product_a, product_b;     /* the species receiving product 3 / product 4; product_b = -1: not tracked (it leaves the box) */
    uint64_t seed;
    uint32_t stream, epoch;
    double   tau, g_lo, g_hi;          /* as fpic_fusion_spec */
    int32_t  n, reserved_i;            /* table entries; zero */
    const double* sigma;               /* n cross-sections, m^2 */
    double   q_value;                  /* J, as fpic_fusion_spectrum_spec */
    double   other_mass;               /* kg: m4 when product_b = -1; zero otherwise */
    double   reserved[4];              /* zero */
} fpic_burn_spec;
typedef struct fpic_burn_result {
    uint64_t applications, pairs, below, above, cells, overfull_cells, overfull_particles, accepted, blocked, saturated, burnt;
    fpic_ionize_gain reactant_a, reactant_b, product_a, product_b;   /* a, b: what the species LOST; the products: GAINED */
} fpic_burn_result;
int fpic_burn(fpic_handle* h, const fpic_burn_spec* spec, fpic_burn_result* out);
int fpic_burn_register(fpic_handle* h, const fpic_burn_spec* spec, int every, int* index);
int fpic_burn_stats(fpic_handle* h, int index, int scope, fpic_burn_result* out);
int fpic_burn_clear(fpic_handle* h);

int fpic_sync(fpic_handle* h);
int fpic_profile(fpic_handle* h, int enable);
int fpic_get_stats(fpic_handle* h, fpic_stats* out);
int fpic_reset_stats(fpic_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* FUSIONPIC_H */
