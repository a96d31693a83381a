/*
 * fusionpic_napi.c — Node N-API (version 8) addon over the C ABI of libfusionpic.so.
 *
 * The reference's host language is JavaScript; its hot path is the object returned
 * by empic.makeCylindricalParticlePusher (empic.js:30-1529).  This addon is the thin
 * native layer under fusion-sim_amd/js/empic_native.js, which re-creates that object
 * with the same method names.  Every function here is one ABI call: it unpacks
 * numbers and typed arrays, calls fpic_*, and converts a non-zero status into a
 * synchronous JavaScript Error carrying fpic_last_error() — the way the reference
 * reports validation and GL failures (utilities.js:118-127, :213-259).
 *
 * Ownership: typed arrays stay owned by JavaScript and are only read or filled
 * during the call.  The native handle is wrapped in an external whose finaliser
 * calls fpic_destroy (napi_add_finalizer semantics), so an unreachable pusher frees
 * its HBM; destroy() does it eagerly.
 */
#include <node_api.h>
#include <stdbool.h>
#include <stdint.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include "fusionpic.h"

#define NAPI_OK(env, call)                                                        \
    do {                                                                          \
        if ((call) != napi_ok) {                                                  \
            napi_throw_error((env), NULL, "N-API call failed: " #call);           \
            return NULL;                                                          \
        }                                                                         \
    } while (0)

#define MAX_SPECIES 16
typedef struct {
    fpic_handle* h;
    size_t n;     /* particle count of the handle: every typed array is checked against the */
    size_t cells; /* size the ABI call will read or write before its pointer is passed on   */
    /* CART3D extension: node count and the particle count of every species */
    size_t nodes;
    int nspecies;
    size_t count[MAX_SPECIES];
    int decomposed;   /* after domainInit count[] is the rank's CAPACITY (domainGetParticles), not a live count */
    /* the request fpic_series_record armed: how many entries a recorded row has (seriesHistory sizes its arrays by them) */
    size_t series_points, series_tracers;
    /* the request fpic_modes_record armed: the doubles of a recorded row (modesHistory sizes its array by them) */
    size_t modes_width;
} box_t;

static void box_finalize(napi_env env, void* data, void* hint)
{
    (void)env; (void)hint;
    box_t* b = (box_t*)data;
    if (b) {
        if (b->h) fpic_destroy(b->h);
        free(b);
    }
}

static napi_value throw_fpic(napi_env env, fpic_handle* h)
{
    const char* msg = fpic_last_error(h);
    napi_throw_error(env, NULL, (msg && *msg) ? msg : "libfusionpic call failed");
    return NULL;
}

static __thread box_t* g_box; /* box of the call being served on this JS thread (set by get_args) */

/* A typed array whose length differs from what the ABI call touches is a RangeError in
 * JavaScript, never a native out-of-bounds access. */
static int check_len(napi_env env, const char* name, size_t len, size_t want)
{
    if (len == want) return 1;
    char msg[160];
    snprintf(msg, sizeof msg, ".%s <- expected a typed array of %zu elements, got %zu", name, want, len);
    napi_throw_range_error(env, NULL, msg);
    return 0;
}

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value* argv, fpic_handle** h)
{
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
        napi_throw_type_error(env, NULL, "wrong number of arguments");
        return 0;
    }
    if (h) {
        box_t* b = NULL;
        if (napi_get_value_external(env, argv[0], (void**)&b) != napi_ok || !b || !b->h) {
            napi_throw_error(env, NULL, "pusher has been destroyed");
            return 0;
        }
        *h = b->h;
        g_box = b;
    }
    return 1;
}

/* The particles species sp of a CART3D box holds NOW, from the library (fpic_population): registered sources and sinks change it
 * inside step(), and fpic_get_particles_of / fpic_get_cells_of write that many rows whatever the caller's array holds — so every
 * caller-order length check asks first.  A rank of a decomposition keeps count[] as its capacity; a library without the symbol
 * (the sanitizer build's stub) keeps the cached count. */
#pragma weak fpic_population
static size_t live_count(fpic_handle* h, int sp)
{
    uint64_t n = 0;
    if (!g_box->decomposed && fpic_population && fpic_population(h, sp, &n, NULL, NULL) == FPIC_OK) {
        g_box->count[sp] = (size_t)n;
        if (sp == 0) g_box->n = (size_t)n;
    }
    return g_box->count[sp];
}

static int get_double(napi_env env, napi_value v, double* out)
{
    if (napi_get_value_double(env, v, out) != napi_ok) {
        napi_throw_type_error(env, NULL, "expected a number");
        return 0;
    }
    return 1;
}

/* Float32Array / Float64Array / Uint8Array / Int32Array or null/undefined. */
static int get_typed(napi_env env, napi_value v, napi_typedarray_type* type, void** data, size_t* length)
{
    napi_valuetype vt;
    *data = NULL; *length = 0;
    if (napi_typeof(env, v, &vt) != napi_ok) return 0;
    if (vt == napi_undefined || vt == napi_null) return 1;
    bool is_ta = false;
    if (napi_is_typedarray(env, v, &is_ta) != napi_ok || !is_ta) {
        napi_throw_type_error(env, NULL, "expected a typed array");
        return 0;
    }
    napi_value ab; size_t off;
    if (napi_get_typedarray_info(env, v, type, length, data, &ab, &off) != napi_ok) {
        napi_throw_type_error(env, NULL, "bad typed array");
        return 0;
    }
    return 1;
}

static int float_dtype(napi_env env, napi_typedarray_type t, int* dtype)
{
    if (t == napi_float32_array) { *dtype = FPIC_F32; return 1; }
    if (t == napi_float64_array) { *dtype = FPIC_F64; return 1; }
    napi_throw_type_error(env, NULL, "expected Float32Array or Float64Array");
    return 0;
}

static napi_value undefined(napi_env env)
{
    napi_value u;
    napi_get_undefined(env, &u);
    return u;
}

/* create(radius, height, nr, nz, dt, nparticles, mass, charge, count, precision, device, physical_a,
 *        sort_interval, unfused_deposit, rng_mode, seed_lo, seed_hi, geometry, solver, ny, length_y, macro_weight, shape,
 *        raster_subpixel_bits) */
static napi_value n_create(napi_env env, napi_callback_info info)
{
    napi_value argv[24];
    if (!get_args(env, info, 24, argv, NULL)) return NULL;
    double d[24];
    for (int i = 0; i < 24; ++i) if (!get_double(env, argv[i], &d[i])) return NULL;
    fpic_spec s;
    memset(&s, 0, sizeof s);
    s.radius = d[0]; s.height = d[1]; s.nr = (int32_t)d[2]; s.nz = (int32_t)d[3]; s.dt = d[4];
    s.nparticles = (int32_t)d[5]; s.particle_mass = d[6]; s.particle_charge = d[7];
    s.count = (uint64_t)d[8]; s.precision = (int32_t)d[9]; s.device = (int32_t)d[10];
    s.physical_a = (int32_t)d[11]; s.sort_interval = (int32_t)d[12]; s.unfused_deposit = (int32_t)d[13];
    s.rng_mode = (int32_t)d[14]; s.rng_seed_lo = (uint32_t)d[15]; s.rng_seed_hi = (uint32_t)d[16];
    s.geometry = (int32_t)d[17]; s.solver = (int32_t)d[18]; s.ny = (int32_t)d[19]; s.length_y = d[20]; s.macro_weight = d[21]; s.shape = (int32_t)d[22];
    s.raster_subpixel_bits = (int32_t)d[23];
    fpic_handle* h = NULL;
    if (fpic_create(&s, &h) != FPIC_OK) return throw_fpic(env, NULL);
    box_t* b = (box_t*)malloc(sizeof *b);
    if (!b) { fpic_destroy(h); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    b->h = h;
    b->n = s.count ? (size_t)s.count : (size_t)s.nparticles * (size_t)s.nparticles;
    b->cells = (size_t)s.nr * (size_t)s.nz;
    b->nodes = b->cells * (size_t)(s.ny > 0 ? s.ny : 1);
    b->nspecies = 1;
    b->count[0] = b->n;
    b->decomposed = 0;
    b->series_points = b->series_tracers = 0;
    b->modes_width = 0;
    napi_value ext;
    if (napi_create_external(env, b, box_finalize, NULL, &ext) != napi_ok) {
        box_finalize(env, b, NULL);
        napi_throw_error(env, NULL, "napi_create_external failed");
        return NULL;
    }
    return ext;
}

static napi_value n_destroy(napi_env env, napi_callback_info info)
{
    napi_value argv[1];
    size_t argc = 1;
    NAPI_OK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
    box_t* b = NULL;
    if (argc == 1 && napi_get_value_external(env, argv[0], (void**)&b) == napi_ok && b && b->h) {
        fpic_destroy(b->h);
        b->h = NULL;
    }
    return undefined(env);
}

/* setParticles(h, positionAoS|null, velocityAoS|null) */
static napi_value n_set_particles(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h;
    if (!get_args(env, info, 3, argv, &h)) return NULL;
    for (int k = 0; k < 2; ++k) {
        napi_typedarray_type t; void* data; size_t len;
        if (!get_typed(env, argv[1 + k], &t, &data, &len)) return NULL;
        if (!data) continue;
        int dtype;
        if (!float_dtype(env, t, &dtype)) return NULL;
        if (len % 3) { napi_throw_error(env, NULL, ".position <- length must be a multiple of 3"); return NULL; }
        if (fpic_set_particles(h, k == 0 ? data : NULL, k == 1 ? data : NULL, len / 3, dtype) != FPIC_OK) return throw_fpic(env, h);
    }
    return undefined(env);
}

/* setGrid(h, which, data, nr, nz, ncomp) */
static napi_value n_set_grid(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h;
    if (!get_args(env, info, 6, argv, &h)) return NULL;
    double which, nr, nz, nc;
    if (!get_double(env, argv[1], &which) || !get_double(env, argv[3], &nr) || !get_double(env, argv[4], &nz) ||
        !get_double(env, argv[5], &nc)) return NULL;
    napi_typedarray_type t; void* data; size_t len; int dtype;
    if (!get_typed(env, argv[2], &t, &data, &len)) return NULL;
    if (!data) { napi_throw_type_error(env, NULL, "expected a typed array"); return NULL; }
    if (!float_dtype(env, t, &dtype)) return NULL;
    if (len != (size_t)(nr * nz * nc)) { napi_throw_error(env, NULL, ".grid <- wrong number of elements"); return NULL; }
    if (fpic_set_grid(h, (int)which, data, (int)nr, (int)nz, (int)nc, dtype) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* setRandomState(h, entropy Float32Array|null, rand Float32Array|null) */
static napi_value n_set_random_state(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h;
    if (!get_args(env, info, 3, argv, &h)) return NULL;
    void* ptr[2] = { NULL, NULL };
    for (int k = 0; k < 2; ++k) {
        napi_typedarray_type t; size_t len;
        if (!get_typed(env, argv[1 + k], &t, &ptr[k], &len)) return NULL;
        if (ptr[k] && t != napi_float32_array) { napi_throw_type_error(env, NULL, "expected Float32Array"); return NULL; }
        if (ptr[k] && k == 0 && len != (size_t)4 * 1024 * 1024) { napi_throw_error(env, NULL, ".entropy <- expected 1024*1024*4 floats"); return NULL; }
        if (ptr[k] && k == 1 && !check_len(env, "rand", len, 4 * g_box->n)) return NULL;
    }
    if (fpic_set_random_state(h, (const float*)ptr[0], (const float*)ptr[1]) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

#define SIMPLE_CALL(NAME, FN)                                                \
    static napi_value NAME(napi_env env, napi_callback_info info)            \
    {                                                                        \
        napi_value argv[1]; fpic_handle* h;                                  \
        if (!get_args(env, info, 1, argv, &h)) return NULL;                  \
        if (FN(h) != FPIC_OK) return throw_fpic(env, h);                     \
        return undefined(env);                                               \
    }
SIMPLE_CALL(n_precalc, fpic_precalc)
SIMPLE_CALL(n_density, fpic_density)
SIMPLE_CALL(n_deposit, fpic_deposit)
SIMPLE_CALL(n_density_finish, fpic_density_finish)
SIMPLE_CALL(n_sort, fpic_sort)
SIMPLE_CALL(n_sync, fpic_sync)
SIMPLE_CALL(n_reset_stats, fpic_reset_stats)

#define DOUBLE_CALL(NAME, FN)                                                \
    static napi_value NAME(napi_env env, napi_callback_info info)            \
    {                                                                        \
        napi_value argv[2]; fpic_handle* h; double v;                        \
        if (!get_args(env, info, 2, argv, &h)) return NULL;                  \
        if (!get_double(env, argv[1], &v)) return NULL;                      \
        if (FN(h, v) != FPIC_OK) return throw_fpic(env, h);                  \
        return undefined(env);                                               \
    }
DOUBLE_CALL(n_add_current_z, fpic_add_current_z)
DOUBLE_CALL(n_add_bz, fpic_add_bz)
DOUBLE_CALL(n_add_btheta, fpic_add_btheta)

static napi_value n_add_current_loop(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; double r, z, c;
    if (!get_args(env, info, 4, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &r) || !get_double(env, argv[2], &z) || !get_double(env, argv[3], &c)) return NULL;
    if (fpic_add_current_loop(h, r, z, c) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

static napi_value n_step(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; double n;
    if (!get_args(env, info, 2, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &n)) return NULL;
    if (fpic_step(h, (int)n) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

static napi_value n_substeps(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; double n;
    if (!get_args(env, info, 2, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &n)) return NULL;
    if (fpic_substeps(h, (int)n) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* stepAsync(h, ncalls) -> Promise: fpic_step + fpic_sync on a libuv worker thread, so that Node's loop is not blocked
 * while the GPU works ("Threading").  The handle is not thread-safe: the shim refuses other calls on the
 * simulation until the promise has settled. */
typedef struct {
    napi_async_work work;
    napi_deferred deferred;
    napi_ref keep;   /* the handle's JS object stays alive (no finaliser) while the step runs */
    fpic_handle* h;
    int ncalls, rc;
    char message[512];
} step_job;

static void step_execute(napi_env env, void* data)
{
    (void)env;
    step_job* j = (step_job*)data;
    j->rc = fpic_step(j->h, j->ncalls);
    if (j->rc == FPIC_OK) j->rc = fpic_sync(j->h);
    if (j->rc != FPIC_OK) {
        const char* m = fpic_last_error(j->h);
        strncpy(j->message, m ? m : "fpic_step failed", sizeof j->message - 1);
        j->message[sizeof j->message - 1] = 0;
    }
}

static void step_complete(napi_env env, napi_status status, void* data)
{
    step_job* j = (step_job*)data;
    napi_value v;
    if (status == napi_ok && j->rc == FPIC_OK) {
        napi_get_undefined(env, &v);
        napi_resolve_deferred(env, j->deferred, v);
    } else {
        napi_value msg;
        napi_create_string_utf8(env, status == napi_ok ? j->message : "the step was cancelled", NAPI_AUTO_LENGTH, &msg);
        napi_create_error(env, NULL, msg, &v);
        napi_reject_deferred(env, j->deferred, v);
    }
    napi_delete_reference(env, j->keep);
    napi_delete_async_work(env, j->work);
    free(j);
}

static napi_value n_step_async(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; double n;
    if (!get_args(env, info, 2, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &n)) return NULL;
    step_job* j = (step_job*)calloc(1, sizeof *j);
    if (!j) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    j->h = h; j->ncalls = (int)n;
    napi_value promise, name;
    if (napi_create_reference(env, argv[0], 1, &j->keep) != napi_ok) { free(j); napi_throw_error(env, NULL, "cannot reference the handle"); return NULL; }
    NAPI_OK(env, napi_create_promise(env, &j->deferred, &promise));
    NAPI_OK(env, napi_create_string_utf8(env, "fusionpic.step", NAPI_AUTO_LENGTH, &name));
    NAPI_OK(env, napi_create_async_work(env, NULL, name, step_execute, step_complete, j, &j->work));
    NAPI_OK(env, napi_queue_async_work(env, j->work));
    return promise;
}

static napi_value n_profile(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; double on;
    if (!get_args(env, info, 2, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &on)) return NULL;
    if (fpic_profile(h, (int)on) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* readGrid(h, which, out Float32Array|Float64Array) */
static napi_value n_read_grid(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double which;
    if (!get_args(env, info, 3, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &which)) return NULL;
    napi_typedarray_type t; void* data; size_t len; int dtype;
    if (!get_typed(env, argv[2], &t, &data, &len)) return NULL;
    if (!data) { napi_throw_type_error(env, NULL, "expected a typed array"); return NULL; }
    if (!float_dtype(env, t, &dtype)) return NULL;
    if (!check_len(env, "out", len, 4 * ((int)which == FPIC_READ_INV_CDF ? (size_t)512 * 512 : g_box->cells))) return NULL;
    if (fpic_read_grid(h, (int)which, data, dtype) != FPIC_OK) return throw_fpic(env, h);
    return argv[2];
}

/* getParticles(h, position|null, velocity|null, rand Float32Array|null, alive Uint8Array|null) */
static napi_value n_get_particles(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h;
    if (!get_args(env, info, 5, argv, &h)) return NULL;
    napi_typedarray_type t[4]; void* p[4]; size_t len[4];
    for (int k = 0; k < 4; ++k) if (!get_typed(env, argv[1 + k], &t[k], &p[k], &len[k])) return NULL;
    int dtype = FPIC_F32;
    if (p[0] && !float_dtype(env, t[0], &dtype)) return NULL;
    if (p[1]) {
        int d2;
        if (!float_dtype(env, t[1], &d2)) return NULL;
        if (p[0] && d2 != dtype) { napi_throw_type_error(env, NULL, "position and velocity must have the same element type"); return NULL; }
        dtype = d2;
    }
    if (p[2] && t[2] != napi_float32_array) { napi_throw_type_error(env, NULL, "rand must be a Float32Array"); return NULL; }
    if (p[3] && t[3] != napi_uint8_array) { napi_throw_type_error(env, NULL, "alive must be a Uint8Array"); return NULL; }
    static const char* const names[4] = { "position", "velocity", "rand", "alive" };
    static const size_t per[4] = { 3, 3, 4, 1 };
    for (int k = 0; k < 4; ++k)
        if (p[k] && !check_len(env, names[k], len[k], per[k] * g_box->n)) return NULL;
    if (fpic_get_particles(h, p[0], p[1], (float*)p[2], (uint8_t*)p[3], dtype) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

static napi_value n_get_cells(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h;
    if (!get_args(env, info, 2, argv, &h)) return NULL;
    napi_typedarray_type t; void* p; size_t len;
    if (!get_typed(env, argv[1], &t, &p, &len)) return NULL;
    if (!p || t != napi_int32_array) { napi_throw_type_error(env, NULL, "expected an Int32Array"); return NULL; }
    if (!check_len(env, "cells", len, g_box->n)) return NULL;
    if (fpic_get_cells(h, (int32_t*)p) != FPIC_OK) return throw_fpic(env, h);
    return argv[1];
}

/* saveCheckpoint(h, path) / loadCheckpoint(h, path) */
static napi_value checkpoint_call(napi_env env, napi_callback_info info, int (*fn)(fpic_handle*, const char*))
{
    napi_value argv[2]; fpic_handle* h;
    if (!get_args(env, info, 2, argv, &h)) return NULL;
    char path[4096]; size_t len = 0;
    if (napi_get_value_string_utf8(env, argv[1], path, sizeof path, &len) != napi_ok) {
        napi_throw_type_error(env, NULL, "expected a path string");
        return NULL;
    }
    if (fn(h, path) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}
static napi_value n_save_checkpoint(napi_env env, napi_callback_info info) { return checkpoint_call(env, info, fpic_save_checkpoint); }
static napi_value n_load_checkpoint(napi_env env, napi_callback_info info) { return checkpoint_call(env, info, fpic_load_checkpoint); }

static napi_value n_get_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    fpic_stats s;
    if (fpic_get_stats(h, &s) != FPIC_OK) return throw_fpic(env, h);
    napi_value o;
    NAPI_OK(env, napi_create_object(env, &o));
    struct { const char* k; double v; } f[] = {
        { "n_particles", (double)s.n_particles }, { "particle_updates", (double)s.particle_updates },
        { "step_launches", (double)s.step_launches }, { "deposit_launches", (double)s.deposit_launches },
        { "sort_passes", (double)s.sort_passes }, { "deposit_spilled", (double)s.deposit_spilled },
        { "ms_push", s.ms_push }, { "ms_deposit", s.ms_deposit }, { "ms_stamp", s.ms_stamp },
        { "ms_precalc", s.ms_precalc }, { "ms_sort", s.ms_sort },
        { "bytes_particle_state", (double)s.bytes_particle_state }, { "bytes_grid_state", (double)s.bytes_grid_state },
    };
    for (size_t i = 0; i < sizeof f / sizeof f[0]; ++i) {
        napi_value v;
        NAPI_OK(env, napi_create_double(env, f[i].v, &v));
        NAPI_OK(env, napi_set_named_property(env, o, f[i].k, v));
    }
    return o;
}

/* ---- CART3D extension (include/fusionpic.h, "extension: spec.geometry") ---- */
static int get_species(napi_env env, napi_value v, int* sp)
{
    double d;
    if (!get_double(env, v, &d)) return 0;
    if (d < 0 || d >= g_box->nspecies) { napi_throw_range_error(env, NULL, ".species <- no such species"); return 0; }
    *sp = (int)d;
    return 1;
}

/* addSpecies(h, mass, charge, count) -> index */
static napi_value n_add_species(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; double m, q, c;
    if (!get_args(env, info, 4, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &m) || !get_double(env, argv[2], &q) || !get_double(env, argv[3], &c)) return NULL;
    if (g_box->nspecies >= MAX_SPECIES) { napi_throw_range_error(env, NULL, ".species <- too many species"); return NULL; }
    int idx = 0;
    if (fpic_add_species(h, m, q, (uint64_t)c, &idx) != FPIC_OK) return throw_fpic(env, h);
    g_box->count[g_box->nspecies++] = (size_t)c;
    napi_value out;
    NAPI_OK(env, napi_create_int32(env, idx, &out));
    return out;
}

/* setParticlesRange(h, species, first, position|null, velocity|null): the caller's particles [first, first + len/3) */
static napi_value n_set_particles_range(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int sp; double first;
    if (!get_args(env, info, 5, argv, &h)) return NULL;
    if (!get_species(env, argv[1], &sp) || !get_double(env, argv[2], &first)) return NULL;
    napi_typedarray_type t[2]; void* p[2]; size_t len[2]; int dtype = -1;
    for (int k = 0; k < 2; ++k) {
        if (!get_typed(env, argv[3 + k], &t[k], &p[k], &len[k])) return NULL;
        if (!p[k]) continue;
        int d2;
        if (!float_dtype(env, t[k], &d2)) return NULL;
        if (dtype >= 0 && d2 != dtype) { napi_throw_type_error(env, NULL, "position and velocity must have the same element type"); return NULL; }
        dtype = d2;
        if (len[k] % 3) { napi_throw_range_error(env, NULL, ".position <- length must be a multiple of 3"); return NULL; }
    }
    if (dtype < 0) return undefined(env);
    if (p[0] && p[1] && len[0] != len[1]) { napi_throw_range_error(env, NULL, ".velocity <- must be as long as .position"); return NULL; }
    const size_t m = (p[0] ? len[0] : len[1]) / 3;
    const size_t live = live_count(h, sp);
    if (first < 0 || (size_t)first > live || m > live - (size_t)first) {
        napi_throw_range_error(env, NULL, ".position <- range lies outside the species");
        return NULL;
    }
    if (fpic_set_particles_range(h, sp, (uint64_t)first, m, p[0], p[1], dtype) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* getParticlesOf(h, species, position|null, velocity|null) */
static napi_value n_get_particles_of(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; int sp;
    if (!get_args(env, info, 4, argv, &h)) return NULL;
    if (!get_species(env, argv[1], &sp)) return NULL;
    napi_typedarray_type t[2]; void* p[2]; size_t len[2]; int dtype = FPIC_F32, have = 0;
    const size_t live = live_count(h, sp);
    for (int k = 0; k < 2; ++k) {
        if (!get_typed(env, argv[2 + k], &t[k], &p[k], &len[k])) return NULL;
        if (!p[k]) continue;
        int d2;
        if (!float_dtype(env, t[k], &d2)) return NULL;
        if (have && d2 != dtype) { napi_throw_type_error(env, NULL, "position and velocity must have the same element type"); return NULL; }
        dtype = d2; have = 1;
        if (!check_len(env, k == 0 ? "position" : "velocity", len[k], 3 * live)) return NULL;
    }
    if (fpic_get_particles_of(h, sp, p[0], p[1], dtype) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* getParticlesRange(h, species, first, stride, position|null, velocity|null): the caller's particles first, first + stride, ...
 * — as many as the arrays hold (len / 3) */
static napi_value n_get_particles_range(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; int sp; double first, stride;
    if (!get_args(env, info, 6, argv, &h)) return NULL;
    if (!get_species(env, argv[1], &sp) || !get_double(env, argv[2], &first) || !get_double(env, argv[3], &stride)) return NULL;
    napi_typedarray_type t[2]; void* p[2]; size_t len[2] = { 0, 0 }; int dtype = -1;
    for (int k = 0; k < 2; ++k) {
        if (!get_typed(env, argv[4 + k], &t[k], &p[k], &len[k])) return NULL;
        if (!p[k]) continue;
        int d2;
        if (!float_dtype(env, t[k], &d2)) return NULL;
        if (dtype >= 0 && d2 != dtype) { napi_throw_type_error(env, NULL, "position and velocity must have the same element type"); return NULL; }
        dtype = d2;
        if (len[k] % 3) { napi_throw_range_error(env, NULL, ".position <- length must be a multiple of 3"); return NULL; }
    }
    if (dtype < 0) return undefined(env);
    if (p[0] && p[1] && len[0] != len[1]) { napi_throw_range_error(env, NULL, ".velocity <- must be as long as .position"); return NULL; }
    const size_t m = (p[0] ? len[0] : len[1]) / 3, have = live_count(h, sp);
    if (first < 0 || stride < 1 || (m && ((size_t)first >= have || (m - 1) > (have - 1 - (size_t)first) / (size_t)stride))) {
        napi_throw_range_error(env, NULL, ".position <- range lies outside the species");
        return NULL;
    }
    if (fpic_get_particles_range(h, sp, (uint64_t)first, m, (uint64_t)stride, p[0], p[1], dtype) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* commInfo(h) -> { rank, world } of the communicator the handle has joined ({0, 1} without one) */
static napi_value n_comm_info(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    int rank = 0, world = 1;
    if (fpic_comm_info(h, &rank, &world) != FPIC_OK) return throw_fpic(env, h);
    napi_value out, v;
    napi_create_object(env, &out);
    napi_create_int32(env, rank, &v); napi_set_named_property(env, out, "rank", v);
    napi_create_int32(env, world, &v); napi_set_named_property(env, out, "world", v);
    return out;
}

static napi_value n_get_cells_of(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; int sp;
    if (!get_args(env, info, 3, argv, &h)) return NULL;
    if (!get_species(env, argv[1], &sp)) return NULL;
    napi_typedarray_type t; void* p; size_t len;
    if (!get_typed(env, argv[2], &t, &p, &len)) return NULL;
    if (!p || t != napi_int32_array) { napi_throw_type_error(env, NULL, "expected an Int32Array"); return NULL; }
    if (!check_len(env, "cells", len, live_count(h, sp))) return NULL;
    if (fpic_get_cells_of(h, sp, (int32_t*)p) != FPIC_OK) return throw_fpic(env, h);
    return argv[2];
}

static napi_value n_add_b(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; double x, y, z;
    if (!get_args(env, info, 4, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &x) || !get_double(env, argv[2], &y) || !get_double(env, argv[3], &z)) return NULL;
    if (fpic_add_b(h, x, y, z) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* setField3(h, which, data, nx, ny, nz) */
static napi_value n_set_field3(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; double which, nx, ny, nz;
    if (!get_args(env, info, 6, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &which) || !get_double(env, argv[3], &nx) || !get_double(env, argv[4], &ny) || !get_double(env, argv[5], &nz)) return NULL;
    napi_typedarray_type t; void* data; size_t len; int dtype;
    if (!get_typed(env, argv[2], &t, &data, &len)) return NULL;
    if (!data) { napi_throw_type_error(env, NULL, "expected a typed array"); return NULL; }
    if (!float_dtype(env, t, &dtype)) return NULL;
    if (!check_len(env, "E", len, (size_t)(nx * ny * nz * 3))) return NULL;
    if (fpic_set_field3(h, (int)which, data, (int)nx, (int)ny, (int)nz, dtype) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* readField3(h, which, out): Float32Array / Float64Array, or BigInt64Array for the fixed-point charge grid */
static napi_value n_read_field3(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double which;
    if (!get_args(env, info, 3, argv, &h)) return NULL;
    if (!get_double(env, argv[1], &which)) return NULL;
    napi_typedarray_type t; void* data; size_t len; int dtype = FPIC_F32;
    if (!get_typed(env, argv[2], &t, &data, &len)) return NULL;
    if (!data) { napi_throw_type_error(env, NULL, "expected a typed array"); return NULL; }
    if ((int)which == FPIC_F3_RHO_FIXED || (int)which == FPIC_F3_J_FIXED) {
        if (t != napi_bigint64_array) { napi_throw_type_error(env, NULL, "expected a BigInt64Array"); return NULL; }
    } else if (!float_dtype(env, t, &dtype)) return NULL;
    if (!check_len(env, "out", len, g_box->nodes * (((int)which == FPIC_F3_RHO || (int)which == FPIC_F3_PHI || (int)which == FPIC_F3_RHO_FIXED) ? 1 : ((int)which == FPIC_F3_J_FIXED ? 3 : 4)))) return NULL;
    if (fpic_read_field3(h, (int)which, data, dtype) != FPIC_OK) return throw_fpic(env, h);
    return argv[2];
}

/* ---- multi-GPU: the library's RCCL communicator ---- */
static napi_value n_comm_unique_id(napi_env env, napi_callback_info info)
{
    (void)info;
    void* data = NULL; napi_value ab, out;
    NAPI_OK(env, napi_create_arraybuffer(env, FPIC_UNIQUE_ID_BYTES, &data, &ab));
    if (fpic_comm_unique_id(data) != FPIC_OK) return throw_fpic(env, NULL);
    NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, FPIC_UNIQUE_ID_BYTES, ab, 0, &out));
    return out;
}

/* commInit(h, id Uint8Array(128), rank, world, overlap) */
static napi_value n_comm_init(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; double rank, world, overlap;
    if (!get_args(env, info, 5, argv, &h)) return NULL;
    napi_typedarray_type t; void* id; size_t len;
    if (!get_typed(env, argv[1], &t, &id, &len)) return NULL;
    if (!id || t != napi_uint8_array) { napi_throw_type_error(env, NULL, "expected a Uint8Array"); return NULL; }
    if (!check_len(env, "id", len, FPIC_UNIQUE_ID_BYTES)) return NULL;
    if (!get_double(env, argv[2], &rank) || !get_double(env, argv[3], &world) || !get_double(env, argv[4], &overlap)) return NULL;
    if (fpic_comm_init(h, id, (int)rank, (int)world) != FPIC_OK) return throw_fpic(env, h);
    if (fpic_comm_set_overlap(h, (int)overlap) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}
SIMPLE_CALL(n_comm_destroy, fpic_comm_destroy)

/* ---- multi-GPU: z-slab decomposition of the box (this process = one rank; exchange over the communicator) ---- */
/* domainInit(h, rank, world, ghostPlanes, migrateEvery, distributedSolve) */
static napi_value n_domain_init(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; double v[5];
    if (!get_args(env, info, 6, argv, &h)) return NULL;
    for (int k = 0; k < 5; ++k)
        if (!get_double(env, argv[1 + k], &v[k])) return NULL;
    if (fpic_domain_init(h, (int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4]) != FPIC_OK) return throw_fpic(env, h);
    g_box->decomposed = 1;
    return undefined(env);
}

/* domainSetParticles(h, species, position, velocity, firstId): the rank's initial particles, global indices firstId.. */
static napi_value n_domain_set_particles(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int sp; double first;
    if (!get_args(env, info, 5, argv, &h)) return NULL;
    if (!get_species(env, argv[1], &sp) || !get_double(env, argv[4], &first)) return NULL;
    napi_typedarray_type t[2]; void* p[2]; size_t len[2]; int d[2];
    for (int k = 0; k < 2; ++k) {
        if (!get_typed(env, argv[2 + k], &t[k], &p[k], &len[k])) return NULL;
        if (!p[k]) { napi_throw_type_error(env, NULL, "expected position and velocity typed arrays"); return NULL; }
        if (!float_dtype(env, t[k], &d[k])) return NULL;
    }
    if (d[0] != d[1]) { napi_throw_type_error(env, NULL, "position and velocity must have the same element type"); return NULL; }
    if (len[0] % 3) { napi_throw_range_error(env, NULL, ".position <- length must be a multiple of 3"); return NULL; }
    if (!check_len(env, "velocity", len[1], len[0])) return NULL;
    if (len[0] / 3 > g_box->count[sp]) { napi_throw_range_error(env, NULL, ".position <- more particles than the species' capacity"); return NULL; }
    if (first < 0 || first > 4294967295.0) { napi_throw_range_error(env, NULL, ".firstId <- must fit 32 bits"); return NULL; }
    if (fpic_domain_set_particles(h, sp, len[0] / 3, p[0], p[1], (uint32_t)first, d[0]) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* domainGetParticles(h, species, position, velocity, ids) -> count; all three sized for the species' capacity */
static napi_value n_domain_get_particles(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int sp;
    if (!get_args(env, info, 5, argv, &h)) return NULL;
    if (!get_species(env, argv[1], &sp)) return NULL;
    napi_typedarray_type t[3]; void* p[3]; size_t len[3]; int d[2];
    for (int k = 0; k < 3; ++k) {
        if (!get_typed(env, argv[2 + k], &t[k], &p[k], &len[k])) return NULL;
        if (!p[k]) { napi_throw_type_error(env, NULL, "expected position, velocity and ids typed arrays"); return NULL; }
    }
    if (!float_dtype(env, t[0], &d[0]) || !float_dtype(env, t[1], &d[1])) return NULL;
    if (d[0] != d[1]) { napi_throw_type_error(env, NULL, "position and velocity must have the same element type"); return NULL; }
    if (t[2] != napi_uint32_array) { napi_throw_type_error(env, NULL, "expected a Uint32Array of ids"); return NULL; }
    if (!check_len(env, "position", len[0], 3 * g_box->count[sp]) || !check_len(env, "velocity", len[1], 3 * g_box->count[sp]) ||
        !check_len(env, "ids", len[2], g_box->count[sp]))
        return NULL;
    uint64_t n = 0;
    if (fpic_domain_get_particles(h, sp, p[0], p[1], (uint32_t*)p[2], g_box->count[sp], &n, d[0]) != FPIC_OK) return throw_fpic(env, h);
    napi_value out;
    NAPI_OK(env, napi_create_double(env, (double)n, &out));
    return out;
}

static napi_value n_domain_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    uint64_t migrated = 0, lost = 0;
    if (fpic_domain_stats(h, &migrated, &lost) != FPIC_OK) return throw_fpic(env, h);
    napi_value out, a, b;
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_create_double(env, (double)migrated, &a));
    NAPI_OK(env, napi_create_double(env, (double)lost, &b));
    NAPI_OK(env, napi_set_named_property(env, out, "migrated", a));
    NAPI_OK(env, napi_set_named_property(env, out, "lost", b));
    return out;
}

/* ---- energy and momentum diagnostics (fpic_energy_*).  One row as an object: the scalars as numbers, the per-species
 * values as Float64Arrays over the box's species (momentum: 3 per species). */
static napi_value energy_object(napi_env env, const fpic_energy* e)
{
    napi_value o, v;
    const int ns = e->nspecies < 0 ? 0 : (e->nspecies > FPIC_ENERGY_SPECIES ? FPIC_ENERGY_SPECIES : e->nspecies);
    NAPI_OK(env, napi_create_object(env, &o));
    struct { const char* k; double v; } f[] = {
        { "substep", (double)e->substep }, { "field_e", e->field_e }, { "field_b", e->field_b }, { "field_b_external", e->field_b_external },
    };
    for (size_t i = 0; i < sizeof f / sizeof f[0]; ++i) {
        NAPI_OK(env, napi_create_double(env, f[i].v, &v));
        NAPI_OK(env, napi_set_named_property(env, o, f[i].k, v));
    }
    const char* names[4] = { "count", "kinetic", "momentum", "speed_max" };
    for (int a = 0; a < 4; ++a) {
        const size_t len = (size_t)ns * (a == 2 ? 3 : 1);
        napi_value buf, arr;
        void* data = NULL;
        NAPI_OK(env, napi_create_arraybuffer(env, len * sizeof(double), &data, &buf));
        double* d = (double*)data;
        for (int s = 0; s < ns; ++s) {
            if (a == 0) d[s] = (double)e->count[s];
            else if (a == 1) d[s] = e->kinetic[s];
            else if (a == 2) { d[3 * s] = e->momentum[s][0]; d[3 * s + 1] = e->momentum[s][1]; d[3 * s + 2] = e->momentum[s][2]; }
            else d[s] = e->speed_max[s];
        }
        NAPI_OK(env, napi_create_typedarray(env, napi_float64_array, len, buf, 0, &arr));
        NAPI_OK(env, napi_set_named_property(env, o, names[a], arr));
    }
    return o;
}

static int get_scope(napi_env env, napi_value v, int* scope)
{
    double d;
    if (!get_double(env, v, &d)) return 0;
    if (d != FPIC_DIAG_LOCAL && d != FPIC_DIAG_GLOBAL) { napi_throw_range_error(env, NULL, ".scope <- must be 0 (local) or 1 (global)"); return 0; }
    *scope = (int)d;
    return 1;
}

/* energy(h, scope) -> row */
static napi_value n_energy(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; int scope;
    if (!get_args(env, info, 2, argv, &h) || !get_scope(env, argv[1], &scope)) return NULL;
    fpic_energy e;
    if (fpic_energy_now(h, scope, &e) != FPIC_OK) return throw_fpic(env, h);
    return energy_object(env, &e);
}

/* recordEnergy(h, every, capacity) */
static napi_value n_record_energy(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double every, cap;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &every) || !get_double(env, argv[2], &cap)) return NULL;
    if (every < 0 || every > 2147483647.0 || cap < 0 || cap > 4294967295.0) { napi_throw_range_error(env, NULL, ".every <- out of range"); return NULL; }
    if (fpic_energy_record(h, (int)every, (uint32_t)cap) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* energyHistory(h, scope) -> { rows: [row, ...], dropped } (the rows recorded since the last call, oldest first) */
static napi_value n_energy_history(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; int scope;
    if (!get_args(env, info, 2, argv, &h) || !get_scope(env, argv[1], &scope)) return NULL;
    uint64_t n = 0, dropped = 0;
    if (fpic_energy_history(h, scope, NULL, 0, &n, &dropped) != FPIC_OK) return throw_fpic(env, h);
    fpic_energy* rows = NULL;
    if (n) {
        rows = (fpic_energy*)calloc((size_t)n, sizeof(fpic_energy));
        if (!rows) { napi_throw_error(env, NULL, "host allocation failed"); return NULL; }
        if (fpic_energy_history(h, scope, rows, n, &n, &dropped) != FPIC_OK) { free(rows); return throw_fpic(env, h); }
    }
    napi_value out, arr, v;
    if (napi_create_object(env, &out) != napi_ok || napi_create_array_with_length(env, (size_t)n, &arr) != napi_ok) { free(rows); return NULL; }
    for (uint64_t i = 0; i < n; ++i) {
        napi_value row = energy_object(env, rows + i);
        if (!row || napi_set_element(env, arr, (uint32_t)i, row) != napi_ok) { free(rows); return NULL; }
    }
    free(rows);
    NAPI_OK(env, napi_set_named_property(env, out, "rows", arr));
    NAPI_OK(env, napi_create_double(env, (double)dropped, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "dropped", v));
    return out;
}

/* histogram(h, species, axes: Int32Array, bins: Int32Array, ranges: Float64Array (lo, hi per axis), scope)
 * -> { counts: BigUint64Array of bins[0] (* bins[1]), outside }.  The arrays' lengths are checked here, the request
 * itself by the library (which is asked before a buffer of the request's size is made). */
static napi_value n_histogram(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; int sp, scope;
    if (!get_args(env, info, 6, argv, &h) || !get_species(env, argv[1], &sp) || !get_scope(env, argv[5], &scope)) return NULL;
    napi_typedarray_type ta, tb, tr; void *pa, *pb, *pr; size_t la, lb, lr;
    if (!get_typed(env, argv[2], &ta, &pa, &la) || !get_typed(env, argv[3], &tb, &pb, &lb) || !get_typed(env, argv[4], &tr, &pr, &lr)) return NULL;
    if (!pa || !pb || !pr || ta != napi_int32_array || tb != napi_int32_array || tr != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".axes <- expected Int32Array axes, Int32Array bins and Float64Array ranges");
        return NULL;
    }
    if (la != 1 && la != 2) { napi_throw_range_error(env, NULL, ".naxes <- must be 1 or 2"); return NULL; }
    if (!check_len(env, "bins", lb, la) || !check_len(env, "range", lr, 2 * la)) return NULL;
    fpic_hist_spec s;
    memset(&s, 0, sizeof s);
    s.species = sp; s.naxes = (int32_t)la;
    uint64_t total = 1;
    for (size_t a = 0; a < la; ++a) {
        s.axis[a] = ((const int32_t*)pa)[a];
        s.bins[a] = ((const int32_t*)pb)[a];
        s.lo[a] = ((const double*)pr)[2 * a];
        s.hi[a] = ((const double*)pr)[2 * a + 1];
        if (s.bins[a] < 1) { napi_throw_range_error(env, NULL, ".bins <- must be at least 1"); return NULL; }
        total *= (uint64_t)s.bins[a];
    }
    if (total > FPIC_HIST_MAX_BINS) { napi_throw_range_error(env, NULL, ".bins <- more than FPIC_HIST_MAX_BINS (2^22) bins in all"); return NULL; }
    napi_value buf, arr, out, v;
    void* data = NULL;
    NAPI_OK(env, napi_create_arraybuffer(env, (size_t)total * sizeof(uint64_t), &data, &buf));
    uint64_t outside = 0;
    if (fpic_histogram(h, &s, scope, (uint64_t*)data, &outside) != FPIC_OK) return throw_fpic(env, h);
    NAPI_OK(env, napi_create_typedarray(env, napi_biguint64_array, (size_t)total, buf, 0, &arr));
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_set_named_property(env, out, "counts", arr));
    NAPI_OK(env, napi_create_double(env, (double)outside, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "outside", v));
    return out;
}

/* the loader's request from words: Float64Array [first, count (-1: to the end), seed low word, seed high word, stream, flags,
 * mode x, y, z] and reals: Float64Array [lo 3, hi 3, drift 3, vth 3, xamp 3, xphase, vamp 3, vphase] (n_load, n_inject*) */
static int load_spec_of(napi_env env, napi_value wv, napi_value rv, int sp, fpic_load_spec* s)
{
    napi_typedarray_type tw, tr; void *pw, *pr; size_t lw, lr;
    if (!get_typed(env, wv, &tw, &pw, &lw) || !get_typed(env, rv, &tr, &pr, &lr)) return 0;
    if (!pw || !pr || tw != napi_float64_array || tr != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".request <- expected two Float64Arrays");
        return 0;
    }
    if (!check_len(env, "words", lw, 9) || !check_len(env, "reals", lr, 20)) return 0;
    const double* w = (const double*)pw;
    const double* r = (const double*)pr;
    const double most[9] = { 18446744073709549568.0, 18446744073709549568.0, 4294967295.0, 4294967295.0, 4294967295.0, 4294967295.0, 2147483647.0, 2147483647.0, 2147483647.0 };
    for (int k = 0; k < 9; ++k) {
        const double least = k == 1 ? -1.0 : (k >= 6 ? -2147483648.0 : 0.0);
        const double mag = w[k] < 0 ? -w[k] : w[k];
        if (!(w[k] >= least && w[k] <= most[k]) || mag != (double)(uint64_t)mag) {
            napi_throw_range_error(env, NULL, ".request <- first, count, seed, stream and mode must be integers within their fields");
            return 0;
        }
    }
    memset(s, 0, sizeof *s);
    s->species = sp;
    s->first = (uint64_t)w[0];
    s->count = w[1] < 0 ? ~(uint64_t)0 : (uint64_t)w[1];
    s->seed = (uint64_t)(uint32_t)w[2] | (uint64_t)(uint32_t)w[3] << 32;
    s->stream = (uint32_t)w[4];
    s->flags = (uint32_t)w[5];
    for (int a = 0; a < 3; ++a) {
        s->mode[a] = (int32_t)w[6 + a];
        s->lo[a] = r[a]; s->hi[a] = r[3 + a]; s->drift[a] = r[6 + a]; s->vth[a] = r[9 + a]; s->xamp[a] = r[12 + a]; s->vamp[a] = r[16 + a];
    }
    s->xphase = r[15]; s->vphase = r[19];
    return 1;
}

/* load(h, species, words: Float64Array [first, count (-1: to the end), seed low word, seed high word, stream, flags, mode x, y, z],
 * reals: Float64Array [lo 3, hi 3, drift 3, vth 3, xamp 3, xphase, vamp 3, vphase]) -> the particles written (kept on a rank of a
 * decomposition).  The arrays' lengths and the words' ranges are checked here, the request itself by the library.
 * load(h, species, words, reals, shape, tables): the same with the tables of a profile (fpic_load_profile; see below). */
static napi_value n_load(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; int sp;
    if (!get_args(env, info, 4, argv, &h) || !get_species(env, argv[1], &sp)) return NULL;
    fpic_load_spec s;
    if (!load_spec_of(env, argv[2], argv[3], sp, &s)) return NULL;
    uint64_t loaded = 0;
    /* the optional tables of a profiled load (fpic_load_profile): shape: Float64Array [density nodes x, y, z, thermal nodes x, y, z,
     * shear nodes, shear axis, shear component], tables: Float64Array, the tables one after the other in that order.  The
     * lengths are checked here, the counts and the values by the library. */
    napi_value more[6];
    size_t argc = 6;
    if (napi_get_cb_info(env, info, &argc, more, NULL, NULL) != napi_ok) return NULL;
    napi_typedarray_type ts = napi_float64_array, tt = napi_float64_array; void *ps = NULL, *pt = NULL; size_t ls = 0, lt = 0;
    if (argc >= 5 && !get_typed(env, more[4], &ts, &ps, &ls)) return NULL;
    if (argc >= 6 && !get_typed(env, more[5], &tt, &pt, &lt)) return NULL;
    if (ps && ls == 11) {
        /* a radial load (fpic_load_radial): shape: Float64Array [geometry, axis, center x, y, z, r_max, density nodes, thermal
         * nodes, radial, azimuthal and axial flow nodes] (eleven entries tell it from a profile's nine), tables: the tables one
         * after the other in that order */
        if (ts != napi_float64_array || (pt && tt != napi_float64_array)) { napi_throw_type_error(env, NULL, ".radial <- expected two Float64Arrays"); return NULL; }
        const double* q = (const double*)ps;
        double total = 0;
        for (int k = 0; k < 11; ++k) {
            if (k >= 2 && k <= 5) continue;
            const double least = k == 1 ? -2147483648.0 : 0.0, most_k = k == 1 ? 2147483647.0 : 4294967295.0;
            if (!(q[k] >= least && q[k] <= most_k) || q[k] != (double)(int64_t)q[k]) {
                napi_throw_range_error(env, NULL, ".radial <- geometry, axis and the node counts must be integers within their fields");
                return NULL;
            }
            if (k >= 6) total += q[k];
        }
        if (!check_len(env, "tables", lt, (size_t)total)) return NULL;
        struct fpic_load_radial p;
        memset(&p, 0, sizeof p);
        const double* at = (const double*)pt;
        p.geometry = (uint32_t)q[0]; p.axis = (int32_t)q[1];
        p.center[0] = q[2]; p.center[1] = q[3]; p.center[2] = q[4]; p.r_max = q[5];
        p.density_n = (uint32_t)q[6]; if (p.density_n) { p.density = at; at += p.density_n; }
        p.thermal_n = (uint32_t)q[7]; if (p.thermal_n) { p.thermal = at; at += p.thermal_n; }
        p.radial_n = (uint32_t)q[8]; if (p.radial_n) { p.radial = at; at += p.radial_n; }
        p.azimuthal_n = (uint32_t)q[9]; if (p.azimuthal_n) { p.azimuthal = at; at += p.azimuthal_n; }
        p.axial_n = (uint32_t)q[10]; if (p.axial_n) p.axial = at;
        if (fpic_load_radial(h, &s, &p, &loaded) != FPIC_OK) return throw_fpic(env, h);
    } else if (ps) {
        if (ts != napi_float64_array || (pt && tt != napi_float64_array)) { napi_throw_type_error(env, NULL, ".profile <- expected two Float64Arrays"); return NULL; }
        if (!check_len(env, "shape", ls, 9)) return NULL;
        const double* q = (const double*)ps;
        double total = 0;
        for (int k = 0; k < 9; ++k) {
            const double least = k >= 7 ? -2147483648.0 : 0.0, most_k = k >= 7 ? 2147483647.0 : 4294967295.0;
            if (!(q[k] >= least && q[k] <= most_k) || q[k] != (double)(int64_t)q[k]) {
                napi_throw_range_error(env, NULL, ".profile <- node counts, shear axis and shear component must be integers within their fields");
                return NULL;
            }
            if (k < 7) total += q[k];
        }
        if (!check_len(env, "tables", lt, (size_t)total)) return NULL;
        struct fpic_load_profile p;
        memset(&p, 0, sizeof p);
        const double* at = (const double*)pt;
        for (int a = 0; a < 3; ++a) { p.density_n[a] = (uint32_t)q[a]; if (p.density_n[a]) { p.density[a] = at; at += p.density_n[a]; } }
        for (int a = 0; a < 3; ++a) { p.thermal_n[a] = (uint32_t)q[3 + a]; if (p.thermal_n[a]) { p.thermal[a] = at; at += p.thermal_n[a]; } }
        p.shear_n = (uint32_t)q[6];
        if (p.shear_n) p.shear = at;
        p.shear_axis = (int32_t)q[7]; p.shear_component = (int32_t)q[8];
        if (fpic_load_profile(h, &s, &p, &loaded) != FPIC_OK) return throw_fpic(env, h);
    } else if (fpic_load(h, &s, &loaded) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_double(env, (double)loaded, &v));
    return v;
}

/* the request of collide / collideEvery: words: Float64Array [kind, seed low word, seed high word, stream, epoch], reals:
 * Float64Array [nu_tau, sigma_tau, g_max, drift 3, vth 3, mass_ratio].  The arrays' lengths and the words' ranges are checked
 * here, the request itself by the library. */
static int get_collide_spec(napi_env env, int sp, napi_value words, napi_value reals, fpic_collide_spec* s)
{
    napi_typedarray_type tw, tr; void *pw, *pr; size_t lw, lr;
    if (!get_typed(env, words, &tw, &pw, &lw) || !get_typed(env, reals, &tr, &pr, &lr)) return 0;
    if (!pw || !pr || tw != napi_float64_array || tr != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".request <- expected two Float64Arrays");
        return 0;
    }
    if (!check_len(env, "words", lw, 5) || !check_len(env, "reals", lr, 10)) return 0;
    const double* w = (const double*)pw;
    const double* r = (const double*)pr;
    for (int k = 0; k < 5; ++k) {
        const double least = k == 0 ? -2147483648.0 : 0.0, most = k == 0 ? 2147483647.0 : 4294967295.0;
        const double mag = w[k] < 0 ? -w[k] : w[k];
        if (!(w[k] >= least && w[k] <= most) || mag != (double)(uint64_t)mag) {
            napi_throw_range_error(env, NULL, ".request <- kind, seed, stream and epoch must be integers within their fields");
            return 0;
        }
    }
    memset(s, 0, sizeof *s);
    s->species = sp;
    s->kind = (int32_t)w[0];
    s->seed = (uint64_t)(uint32_t)w[1] | (uint64_t)(uint32_t)w[2] << 32;
    s->stream = (uint32_t)w[3];
    s->epoch = (uint32_t)w[4];
    s->nu_tau = r[0]; s->sigma_tau = r[1]; s->g_max = r[2];
    for (int a = 0; a < 3; ++a) { s->drift[a] = r[3 + a]; s->vth[a] = r[6 + a]; }
    s->mass_ratio = r[9];
    return 1;
}

static napi_value collide_object(napi_env env, const fpic_collide_result* c)
{
    napi_value o, v;
    const char* names[4] = { "applications", "candidates", "collided", "clipped" };
    const uint64_t vals[4] = { c->applications, c->candidates, c->collided, c->clipped };
    NAPI_OK(env, napi_create_object(env, &o));
    for (int k = 0; k < 4; ++k) {
        NAPI_OK(env, napi_create_double(env, (double)vals[k], &v));
        NAPI_OK(env, napi_set_named_property(env, o, names[k], v));
    }
    return o;
}

/* collide(h, species, words, reals) -> { applications, candidates, collided, clipped } */
static napi_value n_collide(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; int sp;
    fpic_collide_spec s;
    if (!get_args(env, info, 4, argv, &h) || !get_species(env, argv[1], &sp) || !get_collide_spec(env, sp, argv[2], argv[3], &s)) return NULL;
    fpic_collide_result c;
    memset(&c, 0, sizeof c);
    if (fpic_collide(h, &s, &c) != FPIC_OK) return throw_fpic(env, h);
    return collide_object(env, &c);
}

/* collideEvery(h, species, words, reals, every) -> the operator's index */
static napi_value n_collide_every(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int sp; double every;
    fpic_collide_spec s;
    if (!get_args(env, info, 5, argv, &h) || !get_species(env, argv[1], &sp) || !get_collide_spec(env, sp, argv[2], argv[3], &s) || !get_double(env, argv[4], &every)) return NULL;
    if (!(every >= -2147483648.0 && every <= 2147483647.0) || every != (double)(int)every) { napi_throw_range_error(env, NULL, ".every <- must be a 32-bit integer"); return NULL; }
    int index = -1;
    if (fpic_collide_register(h, &s, (int)every, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* collisionStats(h, index, scope) -> { applications, candidates, collided, clipped } */
static napi_value n_collision_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double index; int scope;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &index) || !get_scope(env, argv[2], &scope)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_collide_result c;
    memset(&c, 0, sizeof c);
    if (fpic_collide_stats(h, (int)index, scope, &c) != FPIC_OK) return throw_fpic(env, h);
    return collide_object(env, &c);
}

/* clearCollisions(h) */
static napi_value n_clear_collisions(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_collide_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* the request of force / forceOn: words: Float64Array [kind, nwaves, epoch, start, stop (each 64-bit one as its low and its
 * high 32-bit word), the four waves' modes (12), taper_n (3), envelope_n], reals: Float64Array [lo 3, hi 3, per wave amp 3,
 * nu, phase], tables: Float64Array, the taper tables and the envelope table one after the other.  The arrays' lengths and the
 * words' ranges are checked here, the request itself by the library (which copies the tables during the call). */
#define FORCE_WORDS 24
#define FORCE_REALS 26
static int get_force_spec(napi_env env, int sp, napi_value words, napi_value reals, napi_value tables, fpic_force_spec* s)
{
    napi_typedarray_type tw, tr, tt; void *pw, *pr, *pt; size_t lw, lr, lt;
    if (!get_typed(env, words, &tw, &pw, &lw) || !get_typed(env, reals, &tr, &pr, &lr) || !get_typed(env, tables, &tt, &pt, &lt)) return 0;
    if (!pw || !pr || tw != napi_float64_array || tr != napi_float64_array || tt != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".request <- expected three Float64Arrays");
        return 0;
    }
    if (!check_len(env, "words", lw, FORCE_WORDS) || !check_len(env, "reals", lr, FORCE_REALS)) return 0;
    const double* w = (const double*)pw;
    const double* r = (const double*)pr;
    for (int k = 0; k < FORCE_WORDS; ++k) {
        const int is_signed = k < 2 || (k >= 8 && k < 20);
        const double least = is_signed ? -2147483648.0 : 0.0, most = is_signed ? 2147483647.0 : 4294967295.0;
        const double mag = w[k] < 0 ? -w[k] : w[k];
        if (!(w[k] >= least && w[k] <= most) || mag != (double)(uint64_t)mag) {
            napi_throw_range_error(env, NULL, ".request <- kind, nwaves, epoch, start, stop, mode and the node counts must be integers within their fields");
            return 0;
        }
    }
    memset(s, 0, sizeof *s);
    s->species = sp;
    s->kind = (int32_t)w[0];
    s->nwaves = (int32_t)w[1];
    s->epoch = (uint64_t)(uint32_t)w[2] | (uint64_t)(uint32_t)w[3] << 32;
    s->start = (uint64_t)(uint32_t)w[4] | (uint64_t)(uint32_t)w[5] << 32;
    s->stop = (uint64_t)(uint32_t)w[6] | (uint64_t)(uint32_t)w[7] << 32;
    for (int a = 0; a < 3; ++a) { s->lo[a] = r[a]; s->hi[a] = r[3 + a]; }
    for (int k = 0; k < FPIC_FORCE_MAX_WAVES; ++k) {
        for (int a = 0; a < 3; ++a) { s->wave[k].mode[a] = (int32_t)w[8 + 3 * k + a]; s->wave[k].amp[a] = r[6 + 5 * k + a]; }
        s->wave[k].nu = r[6 + 5 * k + 3];
        s->wave[k].phase = r[6 + 5 * k + 4];
    }
    double total = 0;
    for (int a = 0; a < 4; ++a) total += w[20 + a];
    if (total != (double)lt) {
        napi_throw_range_error(env, NULL, ".tables <- its length must be the sum of the node counts");
        return 0;
    }
    const double* at = (const double*)pt;
    for (int a = 0; a < 3; ++a) {
        s->taper_n[a] = (uint32_t)w[20 + a];
        if (s->taper_n[a]) { s->taper[a] = at; at += s->taper_n[a]; }
    }
    s->envelope_n = (uint32_t)w[23];
    if (s->envelope_n) s->envelope = at;
    return 1;
}

/* a 128-bit two's complement sum (low word, high word) as a BigInt */
static napi_value fixed_bigint(napi_env env, const uint64_t* f)
{
    uint64_t mag[2] = { f[0], f[1] };
    const int neg = (int)(f[1] >> 63);
    if (neg) {
        mag[0] = ~f[0] + 1;
        mag[1] = ~f[1] + (mag[0] == 0 ? 1 : 0);
    }
    napi_value v;
    NAPI_OK(env, napi_create_bigint_words(env, neg, 2, mag, &v));
    return v;
}

static napi_value force_object(napi_env env, const fpic_force_result* c)
{
    napi_value o, v, arr;
    NAPI_OK(env, napi_create_object(env, &o));
    NAPI_OK(env, napi_create_double(env, (double)c->applications, &v));
    NAPI_OK(env, napi_set_named_property(env, o, "applications", v));
    NAPI_OK(env, napi_create_double(env, (double)c->kicked, &v));
    NAPI_OK(env, napi_set_named_property(env, o, "kicked", v));
    v = fixed_bigint(env, c->work_fixed);
    if (!v) return NULL;
    NAPI_OK(env, napi_set_named_property(env, o, "workFixed", v));
    NAPI_OK(env, napi_create_array_with_length(env, 3, &arr));
    for (uint32_t a = 0; a < 3; ++a) {
        v = fixed_bigint(env, c->impulse_fixed[a]);
        if (!v) return NULL;
        NAPI_OK(env, napi_set_element(env, arr, a, v));
    }
    NAPI_OK(env, napi_set_named_property(env, o, "impulseFixed", arr));
    NAPI_OK(env, napi_create_double(env, c->work, &v));
    NAPI_OK(env, napi_set_named_property(env, o, "work", v));
    NAPI_OK(env, napi_create_array_with_length(env, 3, &arr));
    for (uint32_t a = 0; a < 3; ++a) {
        NAPI_OK(env, napi_create_double(env, c->impulse[a], &v));
        NAPI_OK(env, napi_set_element(env, arr, a, v));
    }
    NAPI_OK(env, napi_set_named_property(env, o, "impulse", arr));
    return o;
}

/* force(h, species, words, reals, tables) -> { applications, kicked, workFixed, impulseFixed, work, impulse } */
static napi_value n_force(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int sp;
    fpic_force_spec s;
    if (!get_args(env, info, 5, argv, &h) || !get_species(env, argv[1], &sp) || !get_force_spec(env, sp, argv[2], argv[3], argv[4], &s)) return NULL;
    fpic_force_result c;
    memset(&c, 0, sizeof c);
    if (fpic_force(h, &s, &c) != FPIC_OK) return throw_fpic(env, h);
    return force_object(env, &c);
}

/* forceOn(h, species, words, reals, tables) -> the request's index */
static napi_value n_force_on(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int sp;
    fpic_force_spec s;
    if (!get_args(env, info, 5, argv, &h) || !get_species(env, argv[1], &sp) || !get_force_spec(env, sp, argv[2], argv[3], argv[4], &s)) return NULL;
    int index = -1;
    if (fpic_force_register(h, &s, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* forceStats(h, index, scope) -> { applications, kicked, workFixed, impulseFixed, work, impulse } */
static napi_value n_force_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double index; int scope;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &index) || !get_scope(env, argv[2], &scope)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_force_result c;
    memset(&c, 0, sizeof c);
    if (fpic_force_stats(h, (int)index, scope, &c) != FPIC_OK) return throw_fpic(env, h);
    return force_object(env, &c);
}

/* clearForces(h) */
static napi_value n_clear_forces(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_force_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* the request of collideGas / collideGasEvery: words: Float64Array [kind, seed low word, seed high word, stream, epoch, n,
 * taper_n (3)], reals: Float64Array [density, tau, g_lo, g_hi, drift 3, vth 3, mass_ratio, lo 3, hi 3], tables: Float64Array,
 * the cross-sections and the taper tables one after the other.  The arrays' lengths and the words' ranges are checked here,
 * the request itself by the library (which copies the tables during the call). */
#define GAS_WORDS 9
#define GAS_REALS 17
static int get_gas_spec(napi_env env, int sp, napi_value words, napi_value reals, napi_value tables, fpic_gas_spec* s)
{
    napi_typedarray_type tw, tr, tt; void *pw, *pr, *pt; size_t lw, lr, lt;
    if (!get_typed(env, words, &tw, &pw, &lw) || !get_typed(env, reals, &tr, &pr, &lr) || !get_typed(env, tables, &tt, &pt, &lt)) return 0;
    if (!pw || !pr || tw != napi_float64_array || tr != napi_float64_array || tt != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".request <- expected three Float64Arrays");
        return 0;
    }
    if (!check_len(env, "words", lw, GAS_WORDS) || !check_len(env, "reals", lr, GAS_REALS)) return 0;
    const double* w = (const double*)pw;
    const double* r = (const double*)pr;
    for (int k = 0; k < GAS_WORDS; ++k) {
        const int is_signed = k == 0 || k == 5;
        const double least = is_signed ? -2147483648.0 : 0.0, most = is_signed ? 2147483647.0 : 4294967295.0;
        const double mag = w[k] < 0 ? -w[k] : w[k];
        if (!(w[k] >= least && w[k] <= most) || mag != (double)(uint64_t)mag) {
            napi_throw_range_error(env, NULL, ".request <- kind, seed, stream, epoch and the node counts must be integers within their fields");
            return 0;
        }
    }
    memset(s, 0, sizeof *s);
    s->species = sp;
    s->kind = (int32_t)w[0];
    s->seed = (uint64_t)(uint32_t)w[1] | (uint64_t)(uint32_t)w[2] << 32;
    s->stream = (uint32_t)w[3];
    s->epoch = (uint32_t)w[4];
    s->n = (int32_t)w[5];
    s->density = r[0];
    s->tau = r[1];
    s->g_lo = r[2];
    s->g_hi = r[3];
    for (int a = 0; a < 3; ++a) { s->drift[a] = r[4 + a]; s->vth[a] = r[7 + a]; s->lo[a] = r[11 + a]; s->hi[a] = r[14 + a]; }
    s->mass_ratio = r[10];
    double total = w[5] > 0 ? w[5] : 0;
    for (int a = 0; a < 3; ++a) total += w[6 + a];
    if (total != (double)lt) {
        napi_throw_range_error(env, NULL, ".tables <- its length must be the sum of the node counts");
        return 0;
    }
    const double* at = (const double*)pt;
    if (s->n > 0) { s->sigma = at; at += s->n; }
    for (int a = 0; a < 3; ++a) {
        s->taper_n[a] = (uint32_t)w[6 + a];
        if (s->taper_n[a]) { s->taper[a] = at; at += s->taper_n[a]; }
    }
    return 1;
}

static napi_value gas_object(napi_env env, const fpic_gas_result* c)
{
    napi_value o, v, arr;
    NAPI_OK(env, napi_create_object(env, &o));
    const char* names[5] = { "applications", "candidates", "collided", "below", "above" };
    const uint64_t counts[5] = { c->applications, c->candidates, c->collided, c->below, c->above };
    for (int k = 0; k < 5; ++k) {
        NAPI_OK(env, napi_create_double(env, (double)counts[k], &v));
        NAPI_OK(env, napi_set_named_property(env, o, names[k], v));
    }
    v = fixed_bigint(env, c->energy_fixed);
    if (!v) return NULL;
    NAPI_OK(env, napi_set_named_property(env, o, "energyFixed", v));
    NAPI_OK(env, napi_create_array_with_length(env, 3, &arr));
    for (uint32_t a = 0; a < 3; ++a) {
        v = fixed_bigint(env, c->momentum_fixed[a]);
        if (!v) return NULL;
        NAPI_OK(env, napi_set_element(env, arr, a, v));
    }
    NAPI_OK(env, napi_set_named_property(env, o, "momentumFixed", arr));
    NAPI_OK(env, napi_create_double(env, c->energy, &v));
    NAPI_OK(env, napi_set_named_property(env, o, "energy", v));
    NAPI_OK(env, napi_create_array_with_length(env, 3, &arr));
    for (uint32_t a = 0; a < 3; ++a) {
        NAPI_OK(env, napi_create_double(env, c->momentum[a], &v));
        NAPI_OK(env, napi_set_element(env, arr, a, v));
    }
    NAPI_OK(env, napi_set_named_property(env, o, "momentum", arr));
    return o;
}

/* collideGas(h, species, words, reals, tables) -> { applications, candidates, collided, below, above, energyFixed, momentumFixed, energy, momentum } */
static napi_value n_collide_gas(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int sp;
    fpic_gas_spec s;
    if (!get_args(env, info, 5, argv, &h) || !get_species(env, argv[1], &sp) || !get_gas_spec(env, sp, argv[2], argv[3], argv[4], &s)) return NULL;
    fpic_gas_result c;
    memset(&c, 0, sizeof c);
    if (fpic_gas(h, &s, &c) != FPIC_OK) return throw_fpic(env, h);
    return gas_object(env, &c);
}

/* collideGasEvery(h, species, words, reals, tables, every) -> the operator's index */
static napi_value n_collide_gas_every(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; int sp; double every;
    fpic_gas_spec s;
    if (!get_args(env, info, 6, argv, &h) || !get_species(env, argv[1], &sp) || !get_gas_spec(env, sp, argv[2], argv[3], argv[4], &s) || !get_double(env, argv[5], &every)) return NULL;
    if (!(every >= -2147483648.0 && every <= 2147483647.0) || every != (double)(int)every) { napi_throw_range_error(env, NULL, ".every <- must be a 32-bit integer"); return NULL; }
    int index = -1;
    if (fpic_gas_register(h, &s, (int)every, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* gasStats(h, index, scope) -> as collideGas */
static napi_value n_gas_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double index; int scope;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &index) || !get_scope(env, argv[2], &scope)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_gas_result c;
    memset(&c, 0, sizeof c);
    if (fpic_gas_stats(h, (int)index, scope, &c) != FPIC_OK) return throw_fpic(env, h);
    return gas_object(env, &c);
}

/* clearGas(h) */
static napi_value n_clear_gas(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_gas_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* the request of remove / removeEvery: species, axes: Int32Array, ranges: Float64Array (lo, hi per term), idMod, idRem,
 * outside (0 | 1) — args[1 .. 6].  The arrays' lengths are checked here, the request itself by the library. */
static int get_remove_spec(napi_env env, const napi_value* argv, fpic_remove_spec* s)
{
    int sp; double mod, rem, outside;
    if (!get_species(env, argv[1], &sp) || !get_double(env, argv[4], &mod) || !get_double(env, argv[5], &rem) || !get_double(env, argv[6], &outside)) return 0;
    napi_typedarray_type ta, tr; void *pa, *pr; size_t la, lr;
    if (!get_typed(env, argv[2], &ta, &pa, &la) || !get_typed(env, argv[3], &tr, &pr, &lr)) return 0;
    if ((la && (!pa || !pr)) || ta != napi_int32_array || tr != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".where <- expected Int32Array axes and Float64Array ranges");
        return 0;
    }
    if (la > FPIC_SELECT_MAX_TERMS) { napi_throw_range_error(env, NULL, ".nterms <- must be 0 .. 7"); return 0; }
    if (!check_len(env, "range", lr, 2 * la)) return 0;
    if (!(mod >= 0 && mod <= 4294967295.0 && rem >= 0 && rem <= 4294967295.0) || mod != (double)(uint32_t)mod || rem != (double)(uint32_t)rem) {
        napi_throw_range_error(env, NULL, ".every <- expected [mod, rem] of unsigned 32-bit integers");
        return 0;
    }
    if (outside != 0 && outside != 1) { napi_throw_range_error(env, NULL, ".outside <- must be true or false"); return 0; }
    memset(s, 0, sizeof *s);
    s->species = sp; s->nterms = (int32_t)la;
    for (size_t t = 0; t < la; ++t) {
        s->axis[t] = ((const int32_t*)pa)[t];
        s->lo[t] = ((const double*)pr)[2 * t];
        s->hi[t] = ((const double*)pr)[2 * t + 1];
    }
    s->id_mod = (uint32_t)mod; s->id_rem = (uint32_t)rem;
    s->flags = outside != 0 ? FPIC_REMOVE_OUTSIDE : 0u;
    return 1;
}

/* the object of a sink's or a source's result: its counts under their names, then the exact tallies and their doubles */
static napi_value tally_object(napi_env env, int ncounts, const char* const* names, const uint64_t* counts, const uint64_t* energy_fixed,
                               const uint64_t (*momentum_fixed)[2], double energy, const double* momentum, double charge)
{
    napi_value o, v, arr;
    NAPI_OK(env, napi_create_object(env, &o));
    for (int k = 0; k < ncounts; ++k) {
        NAPI_OK(env, napi_create_double(env, (double)counts[k], &v));
        NAPI_OK(env, napi_set_named_property(env, o, names[k], v));
    }
    v = fixed_bigint(env, energy_fixed);
    if (!v) return NULL;
    NAPI_OK(env, napi_set_named_property(env, o, "energyFixed", v));
    NAPI_OK(env, napi_create_array_with_length(env, 3, &arr));
    for (uint32_t a = 0; a < 3; ++a) {
        v = fixed_bigint(env, momentum_fixed[a]);
        if (!v) return NULL;
        NAPI_OK(env, napi_set_element(env, arr, a, v));
    }
    NAPI_OK(env, napi_set_named_property(env, o, "momentumFixed", arr));
    NAPI_OK(env, napi_create_double(env, energy, &v));
    NAPI_OK(env, napi_set_named_property(env, o, "energy", v));
    NAPI_OK(env, napi_create_array_with_length(env, 3, &arr));
    for (uint32_t a = 0; a < 3; ++a) {
        NAPI_OK(env, napi_create_double(env, momentum[a], &v));
        NAPI_OK(env, napi_set_element(env, arr, a, v));
    }
    NAPI_OK(env, napi_set_named_property(env, o, "momentum", arr));
    NAPI_OK(env, napi_create_double(env, charge, &v));
    NAPI_OK(env, napi_set_named_property(env, o, "charge", v));
    return o;
}

static napi_value remove_object(napi_env env, const fpic_remove_result* c)
{
    const char* names[3] = { "applications", "scanned", "removed" };
    const uint64_t counts[3] = { c->applications, c->scanned, c->removed };
    return tally_object(env, 3, names, counts, c->energy_fixed, c->momentum_fixed, c->energy, c->momentum, c->charge);
}

/* remove(h, species, axes, ranges, idMod, idRem, outside) -> { applications, scanned, removed, energyFixed, momentumFixed, energy, momentum, charge } */
static napi_value n_remove(napi_env env, napi_callback_info info)
{
    napi_value argv[7]; fpic_handle* h;
    fpic_remove_spec s;
    if (!get_args(env, info, 7, argv, &h) || !get_remove_spec(env, argv, &s)) return NULL;
    fpic_remove_result c;
    memset(&c, 0, sizeof c);
    if (fpic_remove(h, &s, &c) != FPIC_OK) return throw_fpic(env, h);
    return remove_object(env, &c);
}

/* removeEvery(h, species, axes, ranges, idMod, idRem, outside, period) -> the operator's index */
static napi_value n_remove_every(napi_env env, napi_callback_info info)
{
    napi_value argv[8]; fpic_handle* h; double every;
    fpic_remove_spec s;
    if (!get_args(env, info, 8, argv, &h) || !get_remove_spec(env, argv, &s) || !get_double(env, argv[7], &every)) return NULL;
    if (!(every >= -2147483648.0 && every <= 2147483647.0) || every != (double)(int)every) { napi_throw_range_error(env, NULL, ".every <- must be a 32-bit integer"); return NULL; }
    int index = -1;
    if (fpic_remove_register(h, &s, (int)every, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* removeStats(h, index, scope) -> as remove */
static napi_value n_remove_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double index; int scope;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &index) || !get_scope(env, argv[2], &scope)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_remove_result c;
    memset(&c, 0, sizeof c);
    if (fpic_remove_stats(h, (int)index, scope, &c) != FPIC_OK) return throw_fpic(env, h);
    return remove_object(env, &c);
}

/* clearRemovals(h) */
static napi_value n_clear_removals(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_remove_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* renumber(h, species) -> the species' particle count */
static napi_value n_renumber(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; int sp;
    if (!get_args(env, info, 2, argv, &h) || !get_species(env, argv[1], &sp)) return NULL;
    uint64_t n = 0;
    if (fpic_renumber(h, sp, &n) != FPIC_OK) return throw_fpic(env, h);
    g_box->count[sp] = (size_t)n;   /* (the caller-order arrays are checked against it from now on) */
    if (sp == 0) g_box->n = (size_t)n;
    napi_value v;
    NAPI_OK(env, napi_create_double(env, (double)n, &v));
    return v;
}

/* ---- particle sources (fpic_reserve, fpic_population, fpic_inject*) */

/* the request of inject / injectEvery: species, words, reals as load takes them, extra: Float64Array [kind, axis, side, plane,
 * epoch low word, epoch high word] */
static int get_inject_spec(napi_env env, const napi_value* argv, fpic_inject_spec* s)
{
    int sp;
    memset(s, 0, sizeof *s);
    if (!get_species(env, argv[1], &sp) || !load_spec_of(env, argv[2], argv[3], sp, &s->load)) return 0;
    napi_typedarray_type te; void* pe; size_t le;
    if (!get_typed(env, argv[4], &te, &pe, &le)) return 0;
    if (!pe || te != napi_float64_array) { napi_throw_type_error(env, NULL, ".request <- expected a Float64Array of the source's own fields"); return 0; }
    if (!check_len(env, "extra", le, 6)) return 0;
    const double* e = (const double*)pe;
    for (int k = 0; k < 6; ++k) {
        if (k == 3) continue;
        const double least = k < 3 ? -2147483648.0 : 0.0, most = k < 3 ? 2147483647.0 : 4294967295.0;
        if (!(e[k] >= least && e[k] <= most) || e[k] != (double)(int64_t)e[k]) {
            napi_throw_range_error(env, NULL, ".request <- kind, axis, side and epoch must be integers within their fields");
            return 0;
        }
    }
    s->kind = (int32_t)e[0]; s->axis = (int32_t)e[1]; s->side = (int32_t)e[2];
    s->plane = e[3];
    s->epoch = (uint64_t)(uint32_t)e[4] | (uint64_t)(uint32_t)e[5] << 32;
    return 1;
}

static napi_value inject_object(napi_env env, const fpic_inject_result* c)
{
    const char* names[2] = { "applications", "injected" };
    const uint64_t counts[2] = { c->applications, c->injected };
    return tally_object(env, 2, names, counts, c->energy_fixed, c->momentum_fixed, c->energy, c->momentum, c->charge);
}

/* inject(h, species, words, reals, extra) -> { applications, injected, energyFixed, momentumFixed, energy, momentum, charge } */
static napi_value n_inject(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h;
    fpic_inject_spec s;
    if (!get_args(env, info, 5, argv, &h) || !get_inject_spec(env, argv, &s)) return NULL;
    fpic_inject_result c;
    memset(&c, 0, sizeof c);
    if (fpic_inject(h, &s, &c) != FPIC_OK) return throw_fpic(env, h);
    (void)live_count(h, s.load.species);
    return inject_object(env, &c);
}

/* injectEvery(h, species, words, reals, extra, period) -> the source's index */
static napi_value n_inject_every(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; double every;
    fpic_inject_spec s;
    if (!get_args(env, info, 6, argv, &h) || !get_inject_spec(env, argv, &s) || !get_double(env, argv[5], &every)) return NULL;
    if (!(every >= -2147483648.0 && every <= 2147483647.0) || every != (double)(int)every) { napi_throw_range_error(env, NULL, ".every <- must be a 32-bit integer"); return NULL; }
    int index = -1;
    if (fpic_inject_register(h, &s, (int)every, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* injectStats(h, index, scope) -> as inject */
static napi_value n_inject_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double index; int scope;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &index) || !get_scope(env, argv[2], &scope)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_inject_result c;
    memset(&c, 0, sizeof c);
    if (fpic_inject_stats(h, (int)index, scope, &c) != FPIC_OK) return throw_fpic(env, h);
    return inject_object(env, &c);
}

/* clearInjections(h) */
static napi_value n_clear_injections(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_inject_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* ---- electron-impact ionisation of a background gas (fpic_ionize*) */

/* the request of ionize / ionizeEvery: species (the projectile), words, reals, tables as collideGas takes them (kind 0, massRatio
 * 0), extra: Float64Array [electron, ion, g_threshold] */
static int get_ionize_spec(napi_env env, const napi_value* argv, fpic_ionize_spec* s)
{
    int sp;
    fpic_gas_spec g;
    if (!get_species(env, argv[1], &sp) || !get_gas_spec(env, sp, argv[2], argv[3], argv[4], &g)) return 0;
    napi_typedarray_type te; void* pe; size_t le;
    if (!get_typed(env, argv[5], &te, &pe, &le)) return 0;
    if (!pe || te != napi_float64_array) { napi_throw_type_error(env, NULL, ".request <- expected a Float64Array of the targets and the threshold"); return 0; }
    if (!check_len(env, "extra", le, 3)) return 0;
    const double* e = (const double*)pe;
    for (int k = 0; k < 2; ++k)
        if (!(e[k] >= -2147483648.0 && e[k] <= 2147483647.0) || e[k] != (double)(int32_t)e[k]) {
            napi_throw_range_error(env, NULL, ".request <- electron and ion must be 32-bit integers");
            return 0;
        }
    memset(s, 0, sizeof *s);
    s->species = g.species;
    s->electron = (int32_t)e[0];
    s->ion = (int32_t)e[1];
    s->g_threshold = e[2];
    s->seed = g.seed; s->stream = g.stream; s->epoch = g.epoch;
    s->density = g.density; s->tau = g.tau; s->g_lo = g.g_lo; s->g_hi = g.g_hi;
    s->n = g.n; s->sigma = g.sigma;
    for (int a = 0; a < 3; ++a) {
        s->drift[a] = g.drift[a]; s->vth[a] = g.vth[a]; s->lo[a] = g.lo[a]; s->hi[a] = g.hi[a];
        s->taper_n[a] = g.taper_n[a]; s->taper[a] = g.taper[a];
    }
    return 1;
}

/* { applications, candidates, below, above, ionised, primary, electron, ion }, each group { energyFixed, momentumFixed, energy,
 * momentum, charge } */
static napi_value ionize_object(napi_env env, const fpic_ionize_result* c)
{
    const char* names[5] = { "applications", "candidates", "below", "above", "ionised" };
    const uint64_t counts[5] = { c->applications, c->candidates, c->below, c->above, c->ionised };
    const fpic_ionize_gain* gains[3] = { &c->primary, &c->electron, &c->ion };
    const char* groups[3] = { "primary", "electron", "ion" };
    napi_value o, v;
    NAPI_OK(env, napi_create_object(env, &o));
    for (int k = 0; k < 5; ++k) {
        NAPI_OK(env, napi_create_double(env, (double)counts[k], &v));
        NAPI_OK(env, napi_set_named_property(env, o, names[k], v));
    }
    for (int k = 0; k < 3; ++k) {
        v = tally_object(env, 0, NULL, NULL, gains[k]->energy_fixed, gains[k]->momentum_fixed, gains[k]->energy, gains[k]->momentum, gains[k]->charge);
        if (!v) return NULL;
        NAPI_OK(env, napi_set_named_property(env, o, groups[k], v));
    }
    return o;
}

/* ionize(h, species, words, reals, tables, extra) -> the result */
static napi_value n_ionize(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h;
    fpic_ionize_spec s;
    if (!get_args(env, info, 6, argv, &h) || !get_ionize_spec(env, argv, &s)) return NULL;
    fpic_ionize_result c;
    memset(&c, 0, sizeof c);
    if (fpic_ionize(h, &s, &c) != FPIC_OK) return throw_fpic(env, h);
    (void)live_count(h, s.electron);          /* (the targets have grown: the caller-order length checks ask the library) */
    (void)live_count(h, s.ion);
    return ionize_object(env, &c);
}

/* ionizeEvery(h, species, words, reals, tables, extra, every) -> the ioniser's index */
static napi_value n_ionize_every(napi_env env, napi_callback_info info)
{
    napi_value argv[7]; fpic_handle* h; double every;
    fpic_ionize_spec s;
    if (!get_args(env, info, 7, argv, &h) || !get_ionize_spec(env, argv, &s) || !get_double(env, argv[6], &every)) return NULL;
    if (!(every >= -2147483648.0 && every <= 2147483647.0) || every != (double)(int)every) { napi_throw_range_error(env, NULL, ".every <- must be a 32-bit integer"); return NULL; }
    int index = -1;
    if (fpic_ionize_register(h, &s, (int)every, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* ionizeStats(h, index, scope) -> as ionize */
static napi_value n_ionize_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double index; int scope;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &index) || !get_scope(env, argv[2], &scope)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_ionize_result c;
    memset(&c, 0, sizeof c);
    if (fpic_ionize_stats(h, (int)index, scope, &c) != FPIC_OK) return throw_fpic(env, h);
    return ionize_object(env, &c);
}

/* clearIonization(h) */
static napi_value n_clear_ionization(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_ionize_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* reserve(h, species, capacity) -> the capacity the species has now */
static napi_value n_reserve(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; int sp; double cap;
    if (!get_args(env, info, 3, argv, &h) || !get_species(env, argv[1], &sp) || !get_double(env, argv[2], &cap)) return NULL;
    if (!(cap >= 0 && cap <= 18446744073709549568.0) || cap != (double)(uint64_t)cap) { napi_throw_range_error(env, NULL, ".capacity <- must be a non-negative integer"); return NULL; }
    uint64_t got = 0;
    if (fpic_reserve(h, sp, (uint64_t)cap, &got) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_double(env, (double)got, &v));
    return v;
}

/* population(h, species) -> { n, capacity, id_span } */
static napi_value n_population(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; int sp;
    if (!get_args(env, info, 2, argv, &h) || !get_species(env, argv[1], &sp)) return NULL;
    uint64_t w[3] = { 0, 0, 0 };
    if (!fpic_population) { napi_throw_error(env, NULL, "this libfusionpic has no fpic_population"); return NULL; }
    if (fpic_population(h, sp, &w[0], &w[1], &w[2]) != FPIC_OK) return throw_fpic(env, h);
    (void)live_count(h, sp);   /* (a rank of a decomposition keeps count[] as its capacity) */
    const char* names[3] = { "n", "capacity", "id_span" };
    napi_value o, v;
    NAPI_OK(env, napi_create_object(env, &o));
    for (int k = 0; k < 3; ++k) {
        NAPI_OK(env, napi_create_double(env, (double)w[k], &v));
        NAPI_OK(env, napi_set_named_property(env, o, names[k], v));
    }
    return o;
}

/* the request of collidePair / collidePairEvery: words: Float64Array [species_a, species_b, seed low word, seed high word,
 * stream, epoch], reals: Float64Array [log_lambda, tau].  The arrays' lengths and the words' ranges are checked here, the
 * request itself by the library. */
static int get_pair_spec(napi_env env, napi_value words, napi_value reals, fpic_pair_spec* s)
{
    napi_typedarray_type tw, tr; void *pw, *pr; size_t lw, lr;
    if (!get_typed(env, words, &tw, &pw, &lw) || !get_typed(env, reals, &tr, &pr, &lr)) return 0;
    if (!pw || !pr || tw != napi_float64_array || tr != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".request <- expected two Float64Arrays");
        return 0;
    }
    if (!check_len(env, "words", lw, 6) || !check_len(env, "reals", lr, 2)) return 0;
    const double* w = (const double*)pw;
    const double* r = (const double*)pr;
    for (int k = 0; k < 6; ++k) {
        const double least = k < 2 ? -2147483648.0 : 0.0, most = k < 2 ? 2147483647.0 : 4294967295.0;
        const double mag = w[k] < 0 ? -w[k] : w[k];
        if (!(w[k] >= least && w[k] <= most) || mag != (double)(uint64_t)mag) {
            napi_throw_range_error(env, NULL, ".request <- a, b, seed, stream and epoch must be integers within their fields");
            return 0;
        }
    }
    memset(s, 0, sizeof *s);
    s->species_a = (int32_t)w[0];
    s->species_b = (int32_t)w[1];
    s->seed = (uint64_t)(uint32_t)w[2] | (uint64_t)(uint32_t)w[3] << 32;
    s->stream = (uint32_t)w[4];
    s->epoch = (uint32_t)w[5];
    s->log_lambda = r[0];
    s->tau = r[1];
    return 1;
}

static napi_value pair_object(napi_env env, const fpic_pair_result* c)
{
    napi_value o, v;
    const char* names[6] = { "applications", "pairs", "strong", "cells", "overfullCells", "overfullParticles" };
    const uint64_t vals[6] = { c->applications, c->pairs, c->strong, c->cells, c->overfull_cells, c->overfull_particles };
    NAPI_OK(env, napi_create_object(env, &o));
    for (int k = 0; k < 6; ++k) {
        NAPI_OK(env, napi_create_double(env, (double)vals[k], &v));
        NAPI_OK(env, napi_set_named_property(env, o, names[k], v));
    }
    return o;
}

/* collidePair(h, words, reals) -> { applications, pairs, strong, cells, overfullCells, overfullParticles } */
static napi_value n_collide_pair(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h;
    fpic_pair_spec s;
    if (!get_args(env, info, 3, argv, &h) || !get_pair_spec(env, argv[1], argv[2], &s)) return NULL;
    fpic_pair_result c;
    memset(&c, 0, sizeof c);
    if (fpic_pair(h, &s, &c) != FPIC_OK) return throw_fpic(env, h);
    return pair_object(env, &c);
}

/* collidePairEvery(h, words, reals, every) -> the operator's index */
static napi_value n_collide_pair_every(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; double every;
    fpic_pair_spec s;
    if (!get_args(env, info, 4, argv, &h) || !get_pair_spec(env, argv[1], argv[2], &s) || !get_double(env, argv[3], &every)) return NULL;
    if (!(every >= -2147483648.0 && every <= 2147483647.0) || every != (double)(int)every) { napi_throw_range_error(env, NULL, ".every <- must be a 32-bit integer"); return NULL; }
    int index = -1;
    if (fpic_pair_register(h, &s, (int)every, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* pairStats(h, index, scope) -> the totals of a registered operator */
static napi_value n_pair_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double index; int scope;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &index) || !get_scope(env, argv[2], &scope)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_pair_result c;
    memset(&c, 0, sizeof c);
    if (fpic_pair_stats(h, (int)index, scope, &c) != FPIC_OK) return throw_fpic(env, h);
    return pair_object(env, &c);
}

/* clearPairs(h) */
static napi_value n_clear_pairs(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_pair_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* the request of fusionYield / fusionYieldEvery: words: Float64Array [species_a, species_b, seed low word, seed high word,
 * stream, epoch], reals: Float64Array [tau, g_lo, g_hi], sigma: Float64Array of 2 .. FPIC_FUSION_TABLE_MAX cross-sections
 * (the request points into it: it lives as long as the call).  The arrays' types and lengths and the words' ranges are
 * checked here, the request itself by the library. */
static int get_fusion_spec(napi_env env, napi_value words, napi_value reals, napi_value sigma, fpic_fusion_spec* s)
{
    napi_typedarray_type tw, tr, ts; void *pw, *pr, *ps; size_t lw, lr, ls;
    if (!get_typed(env, words, &tw, &pw, &lw) || !get_typed(env, reals, &tr, &pr, &lr) || !get_typed(env, sigma, &ts, &ps, &ls)) return 0;
    if (!pw || !pr || tw != napi_float64_array || tr != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".request <- expected two Float64Arrays");
        return 0;
    }
    if (!ps || ts != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".sigma <- expected a Float64Array");
        return 0;
    }
    if (!check_len(env, "words", lw, 6) || !check_len(env, "reals", lr, 3)) return 0;
    if (ls < 2 || ls > FPIC_FUSION_TABLE_MAX) {
        napi_throw_range_error(env, NULL, ".n <- must be 2 .. FPIC_FUSION_TABLE_MAX (4096)");
        return 0;
    }
    const double* w = (const double*)pw;
    const double* r = (const double*)pr;
    for (int k = 0; k < 6; ++k) {
        const double least = k < 2 ? -2147483648.0 : 0.0, most = k < 2 ? 2147483647.0 : 4294967295.0;
        const double mag = w[k] < 0 ? -w[k] : w[k];
        if (!(w[k] >= least && w[k] <= most) || mag != (double)(uint64_t)mag) {
            napi_throw_range_error(env, NULL, ".request <- a, b, seed, stream and epoch must be integers within their fields");
            return 0;
        }
    }
    memset(s, 0, sizeof *s);
    s->species_a = (int32_t)w[0];
    s->species_b = (int32_t)w[1];
    s->seed = (uint64_t)(uint32_t)w[2] | (uint64_t)(uint32_t)w[3] << 32;
    s->stream = (uint32_t)w[4];
    s->epoch = (uint32_t)w[5];
    s->tau = r[0];
    s->g_lo = r[1];
    s->g_hi = r[2];
    s->n = (int32_t)ls;
    s->sigma = (const double*)ps;
    return 1;
}

/* a BigInt64Array of the box's cells, or null / undefined (*data = NULL) */
static int get_fusion_grid(napi_env env, napi_value v, int64_t** data)
{
    napi_typedarray_type t; void* p; size_t len;
    *data = NULL;
    if (!get_typed(env, v, &t, &p, &len)) return 0;
    if (!p && !len) return 1;
    if (!p || t != napi_bigint64_array) { napi_throw_type_error(env, NULL, ".grid <- expected a BigInt64Array"); return 0; }
    if (!check_len(env, "grid", len, g_box->nodes)) return 0;
    *data = (int64_t*)p;
    return 1;
}

/* the counts; the total yield_hi 2^32 + yield_lo travels as three exact numbers (yieldTop = yield_hi >> 32, yieldMid = its low
 * word, yieldLo), which the shim joins into a BigInt */
static napi_value fusion_object(napi_env env, const fpic_fusion_result* c)
{
    napi_value o, v;
    const char* names[11] = { "applications", "pairs", "below", "above", "cells", "overfullCells", "overfullParticles", "yieldTop", "yieldMid", "yieldLo", "unitExponent" };
    const double vals[11] = { (double)c->applications, (double)c->pairs, (double)c->below, (double)c->above, (double)c->cells, (double)c->overfull_cells,
                              (double)c->overfull_particles, (double)(c->yield_hi >> 32), (double)(c->yield_hi & 0xFFFFFFFFull), (double)c->yield_lo, (double)c->unit_exponent };
    NAPI_OK(env, napi_create_object(env, &o));
    for (int k = 0; k < 11; ++k) {
        NAPI_OK(env, napi_create_double(env, vals[k], &v));
        NAPI_OK(env, napi_set_named_property(env, o, names[k], v));
    }
    return o;
}

/* fusionYield(h, words, reals, sigma, grid: BigInt64Array of the cells or null) -> the counts */
static napi_value n_fusion_yield(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int64_t* grid;
    fpic_fusion_spec s;
    if (!get_args(env, info, 5, argv, &h) || !get_fusion_spec(env, argv[1], argv[2], argv[3], &s) || !get_fusion_grid(env, argv[4], &grid)) return NULL;
    fpic_fusion_result c;
    memset(&c, 0, sizeof c);
    if (fpic_fusion(h, &s, &c, grid) != FPIC_OK) return throw_fpic(env, h);
    return fusion_object(env, &c);
}

/* fusionYieldEvery(h, words, reals, sigma, every) -> the operator's index */
static napi_value n_fusion_yield_every(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; double every;
    fpic_fusion_spec s;
    if (!get_args(env, info, 5, argv, &h) || !get_fusion_spec(env, argv[1], argv[2], argv[3], &s) || !get_double(env, argv[4], &every)) return NULL;
    if (!(every >= -2147483648.0 && every <= 2147483647.0) || every != (double)(int)every) { napi_throw_range_error(env, NULL, ".every <- must be a 32-bit integer"); return NULL; }
    int index = -1;
    if (fpic_fusion_register(h, &s, (int)every, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* fusionStats(h, index, scope) -> the totals of a registered tally */
static napi_value n_fusion_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double index; int scope;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &index) || !get_scope(env, argv[2], &scope)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_fusion_result c;
    memset(&c, 0, sizeof c);
    if (fpic_fusion_stats(h, (int)index, scope, &c) != FPIC_OK) return throw_fpic(env, h);
    return fusion_object(env, &c);
}

/* fusionGrid(h, index, grid: BigInt64Array of the cells or null, reset: 0 or 1) */
static napi_value n_fusion_grid(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; double index, reset; int64_t* grid;
    if (!get_args(env, info, 4, argv, &h) || !get_double(env, argv[1], &index) || !get_fusion_grid(env, argv[2], &grid) || !get_double(env, argv[3], &reset)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    if (fpic_fusion_grid(h, (int)index, grid, reset != 0) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* clearFusion(h) */
static napi_value n_clear_fusion(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_fusion_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* ---- fusion burn: reactants consumed, products born (fpic_burn*) */

/* the request of burn / burnEvery: words, reals, sigma as fusionYield takes them, extra: Float64Array [product_a, product_b
 * (-1: not tracked), q_value, other_mass] */
static int get_burn_spec(napi_env env, const napi_value* argv, fpic_burn_spec* s)
{
    fpic_fusion_spec f;
    if (!get_fusion_spec(env, argv[1], argv[2], argv[3], &f)) return 0;
    napi_typedarray_type te; void* pe; size_t le;
    if (!get_typed(env, argv[4], &te, &pe, &le)) return 0;
    if (!pe || te != napi_float64_array) { napi_throw_type_error(env, NULL, ".request <- expected a Float64Array of the products, the q-value and the other mass"); return 0; }
    if (!check_len(env, "extra", le, 4)) return 0;
    const double* e = (const double*)pe;
    for (int k = 0; k < 2; ++k)
        if (!(e[k] >= -2147483648.0 && e[k] <= 2147483647.0) || e[k] != (double)(int32_t)e[k]) {
            napi_throw_range_error(env, NULL, ".request <- the products must be 32-bit integers");
            return 0;
        }
    memset(s, 0, sizeof *s);
    s->species_a = f.species_a; s->species_b = f.species_b;
    s->product_a = (int32_t)e[0]; s->product_b = (int32_t)e[1];
    s->seed = f.seed; s->stream = f.stream; s->epoch = f.epoch;
    s->tau = f.tau; s->g_lo = f.g_lo; s->g_hi = f.g_hi;
    s->n = f.n; s->sigma = f.sigma;
    s->q_value = e[2];
    s->other_mass = e[3];
    return 1;
}

/* { applications, pairs, below, above, cells, overfullCells, overfullParticles, accepted, blocked, saturated, burnt, reactantA,
 * reactantB, productA, productB }, each group { energyFixed, momentumFixed, energy, momentum, charge } */
static napi_value burn_object(napi_env env, const fpic_burn_result* c)
{
    const char* names[11] = { "applications", "pairs", "below", "above", "cells", "overfullCells", "overfullParticles", "accepted", "blocked", "saturated", "burnt" };
    const uint64_t counts[11] = { c->applications, c->pairs, c->below, c->above, c->cells, c->overfull_cells, c->overfull_particles, c->accepted, c->blocked, c->saturated, c->burnt };
    const fpic_ionize_gain* gains[4] = { &c->reactant_a, &c->reactant_b, &c->product_a, &c->product_b };
    const char* groups[4] = { "reactantA", "reactantB", "productA", "productB" };
    napi_value o, v;
    NAPI_OK(env, napi_create_object(env, &o));
    for (int k = 0; k < 11; ++k) {
        NAPI_OK(env, napi_create_double(env, (double)counts[k], &v));
        NAPI_OK(env, napi_set_named_property(env, o, names[k], v));
    }
    for (int k = 0; k < 4; ++k) {
        v = tally_object(env, 0, NULL, NULL, gains[k]->energy_fixed, gains[k]->momentum_fixed, gains[k]->energy, gains[k]->momentum, gains[k]->charge);
        if (!v) return NULL;
        NAPI_OK(env, napi_set_named_property(env, o, groups[k], v));
    }
    return o;
}

/* burn(h, words, reals, sigma, extra) -> the result */
static napi_value n_burn(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h;
    fpic_burn_spec s;
    if (!get_args(env, info, 5, argv, &h) || !get_burn_spec(env, argv, &s)) return NULL;
    fpic_burn_result c;
    memset(&c, 0, sizeof c);
    if (fpic_burn(h, &s, &c) != FPIC_OK) return throw_fpic(env, h);
    (void)live_count(h, s.species_a);         /* (every species of the request has changed: the caller-order length checks ask the library) */
    (void)live_count(h, s.species_b);
    (void)live_count(h, s.product_a);
    if (s.product_b >= 0) (void)live_count(h, s.product_b);
    return burn_object(env, &c);
}

/* burnEvery(h, words, reals, sigma, extra, every) -> the burner's index */
static napi_value n_burn_every(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; double every;
    fpic_burn_spec s;
    if (!get_args(env, info, 6, argv, &h) || !get_burn_spec(env, argv, &s) || !get_double(env, argv[5], &every)) return NULL;
    if (!(every >= -2147483648.0 && every <= 2147483647.0) || every != (double)(int)every) { napi_throw_range_error(env, NULL, ".every <- must be a 32-bit integer"); return NULL; }
    int index = -1;
    if (fpic_burn_register(h, &s, (int)every, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* burnStats(h, index, scope) -> as burn */
static napi_value n_burn_stats(napi_env env, napi_callback_info info)
{
    napi_value argv[3]; fpic_handle* h; double index; int scope;
    if (!get_args(env, info, 3, argv, &h) || !get_double(env, argv[1], &index) || !get_scope(env, argv[2], &scope)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_burn_result c;
    memset(&c, 0, sizeof c);
    if (fpic_burn_stats(h, (int)index, scope, &c) != FPIC_OK) return throw_fpic(env, h);
    return burn_object(env, &c);
}

/* clearBurn(h) */
static napi_value n_clear_burn(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_burn_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* the request of fusionSpectrum / fusionSpectrumEvery: the tally's three arrays (get_fusion_spec) and axis: Float64Array
 * [axis, bins, lo, hi, q_value, product_mass, other_mass, los x, los y, los z].  The array's type and length and the two
 * integers' ranges are checked here, the request itself by the library. */
static int get_fusion_spectrum_spec(napi_env env, napi_value words, napi_value reals, napi_value sigma, napi_value axis, fpic_fusion_spectrum_spec* s)
{
    memset(s, 0, sizeof *s);
    if (!get_fusion_spec(env, words, reals, sigma, &s->tally)) return 0;
    napi_typedarray_type t; void* p; size_t len;
    if (!get_typed(env, axis, &t, &p, &len)) return 0;
    if (!p || t != napi_float64_array) { napi_throw_type_error(env, NULL, ".axis <- expected a Float64Array"); return 0; }
    if (!check_len(env, "axis", len, 10)) return 0;
    const double* a = (const double*)p;
    for (int k = 0; k < 2; ++k)
        if (!(a[k] >= -2147483648.0 && a[k] <= 2147483647.0) || a[k] != (double)(int)a[k]) {
            napi_throw_range_error(env, NULL, ".axis <- axis and bins must be 32-bit integers");
            return 0;
        }
    s->axis = (int32_t)a[0];
    s->bins = (int32_t)a[1];
    s->lo = a[2];
    s->hi = a[3];
    s->q_value = a[4];
    s->product_mass = a[5];
    s->other_mass = a[6];
    for (int k = 0; k < 3; ++k) s->los[k] = a[7 + k];
    return 1;
}

/* a BigUint64Array of `entries` x 2 words, or null / undefined (*data = NULL) */
static int get_fusion_words(napi_env env, napi_value v, size_t entries, uint64_t** data)
{
    napi_typedarray_type t; void* p; size_t len;
    *data = NULL;
    if (!get_typed(env, v, &t, &p, &len)) return 0;
    if (!p && !len) return 1;
    if (!p || t != napi_biguint64_array) { napi_throw_type_error(env, NULL, ".words <- expected a BigUint64Array"); return 0; }
    if (!check_len(env, "words", len, 2 * entries)) return 0;
    *data = (uint64_t*)p;
    return 1;
}

/* fusionSpectrum(h, words, reals, sigma, axis, out: BigUint64Array of (bins + 2) x 2 words or null) -> the counts */
static napi_value n_fusion_spectrum(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; uint64_t* out;
    fpic_fusion_spectrum_spec s;
    if (!get_args(env, info, 6, argv, &h) || !get_fusion_spectrum_spec(env, argv[1], argv[2], argv[3], argv[4], &s)) return NULL;
    if (s.bins < 1 || s.bins > FPIC_FUSION_SPECTRUM_BINS_MAX) { napi_throw_range_error(env, NULL, ".bins <- must be 1 .. FPIC_FUSION_SPECTRUM_BINS_MAX (256)"); return NULL; }
    if (!get_fusion_words(env, argv[5], (size_t)s.bins + 2, &out)) return NULL;
    fpic_fusion_result c;
    memset(&c, 0, sizeof c);
    if (fpic_fusion_spectrum(h, &s, &c, out) != FPIC_OK) return throw_fpic(env, h);
    return fusion_object(env, &c);
}

/* fusionSpectrumEvery(h, words, reals, sigma, axis, every) -> the operator's index */
static napi_value n_fusion_spectrum_every(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; double every;
    fpic_fusion_spectrum_spec s;
    if (!get_args(env, info, 6, argv, &h) || !get_fusion_spectrum_spec(env, argv[1], argv[2], argv[3], argv[4], &s) || !get_double(env, argv[5], &every)) return NULL;
    if (!(every >= -2147483648.0 && every <= 2147483647.0) || every != (double)(int)every) { napi_throw_range_error(env, NULL, ".every <- must be a 32-bit integer"); return NULL; }
    int index = -1;
    if (fpic_fusion_spectrum_register(h, &s, (int)every, &index) != FPIC_OK) return throw_fpic(env, h);
    napi_value v;
    NAPI_OK(env, napi_create_int32(env, index, &v));
    return v;
}

/* fusionSpectrumRead(h, index, out: BigUint64Array of (FPIC_FUSION_SPECTRUM_BINS_MAX + 2) x 2 words or null, reset: 0 or 1) ->
 * the counts.  Only the library knows the operator's bins, so the array always has room for the cap: the first
 * (bins + 2) x 2 words are written. */
static napi_value n_fusion_spectrum_read(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; double index, reset; uint64_t* out;
    if (!get_args(env, info, 4, argv, &h) || !get_double(env, argv[1], &index) || !get_fusion_words(env, argv[2], FPIC_FUSION_SPECTRUM_BINS_MAX + 2, &out) ||
        !get_double(env, argv[3], &reset)) return NULL;
    if (!(index >= -2147483648.0 && index <= 2147483647.0) || index != (double)(int)index) { napi_throw_range_error(env, NULL, ".index <- must be a 32-bit integer"); return NULL; }
    fpic_fusion_result c;
    memset(&c, 0, sizeof c);
    if (fpic_fusion_spectrum_read(h, (int)index, &c, out, reset != 0) != FPIC_OK) return throw_fpic(env, h);
    return fusion_object(env, &c);
}

/* clearFusionSpectra(h) */
static napi_value n_clear_fusion_spectra(napi_env env, napi_callback_info info)
{
    napi_value argv[1]; fpic_handle* h;
    if (!get_args(env, info, 1, argv, &h)) return NULL;
    if (fpic_fusion_spectrum_clear(h) != FPIC_OK) return throw_fpic(env, h);
    return undefined(env);
}

/* select(h, species, axes: Int32Array, ranges: Float64Array (lo, hi per term), idMod, idRem, capacity, dtype (0: Float32Array,
 * 1: Float64Array), scope) -> { ids: Uint32Array, position, velocity, matched }.  capacity < 0: the count query first, then a
 * call with room for exactly that many rows; capacity 0: the count query alone.  The three arrays are null when `matched`
 * exceeds a given capacity.  The arrays' lengths are checked here, the request itself by the library. */
static napi_value n_select(napi_env env, napi_callback_info info)
{
    napi_value argv[9]; fpic_handle* h; int sp, scope; double mod, rem, cap, dt;
    if (!get_args(env, info, 9, argv, &h) || !get_species(env, argv[1], &sp) || !get_double(env, argv[4], &mod) || !get_double(env, argv[5], &rem) ||
        !get_double(env, argv[6], &cap) || !get_double(env, argv[7], &dt) || !get_scope(env, argv[8], &scope)) return NULL;
    napi_typedarray_type ta, tr; void *pa, *pr; size_t la, lr;
    if (!get_typed(env, argv[2], &ta, &pa, &la) || !get_typed(env, argv[3], &tr, &pr, &lr)) return NULL;
    if ((la && (!pa || !pr)) || ta != napi_int32_array || tr != napi_float64_array) {
        napi_throw_type_error(env, NULL, ".where <- expected Int32Array axes and Float64Array ranges");
        return NULL;
    }
    if (la > FPIC_SELECT_MAX_TERMS) { napi_throw_range_error(env, NULL, ".nterms <- must be 0 .. 7"); return NULL; }
    if (!check_len(env, "range", lr, 2 * la)) return NULL;
    if (!(mod >= 0 && mod <= 4294967295.0 && rem >= 0 && rem <= 4294967295.0) || mod != (double)(uint32_t)mod || rem != (double)(uint32_t)rem) {
        napi_throw_range_error(env, NULL, ".every <- expected [mod, rem] of unsigned 32-bit integers");
        return NULL;
    }
    if (!(cap >= -1 && cap <= (double)FPIC_SELECT_MAX_ROWS) || cap != (double)(int64_t)cap) {
        napi_throw_range_error(env, NULL, ".capacity <- more than FPIC_SELECT_MAX_ROWS (2^24) rows, or not an integer");
        return NULL;
    }
    if (dt != 0 && dt != 1) { napi_throw_range_error(env, NULL, ".dtype <- must be 0 (f32) or 1 (f64)"); return NULL; }
    fpic_select_spec s;
    memset(&s, 0, sizeof s);
    s.species = sp; s.nterms = (int32_t)la;
    for (size_t t = 0; t < la; ++t) {
        s.axis[t] = ((const int32_t*)pa)[t];
        s.lo[t] = ((const double*)pr)[2 * t];
        s.hi[t] = ((const double*)pr)[2 * t + 1];
    }
    s.id_mod = (uint32_t)mod; s.id_rem = (uint32_t)rem;
    const int dtype = dt == 0 ? FPIC_F32 : FPIC_F64;
    uint64_t matched = 0, capacity = cap < 0 ? 0 : (uint64_t)cap;
    if (cap < 0) {
        if (fpic_select(h, &s, scope, 0, NULL, NULL, NULL, dtype, &matched) != FPIC_OK) return throw_fpic(env, h);
        if (matched > FPIC_SELECT_MAX_ROWS) { napi_throw_range_error(env, NULL, ".capacity <- more than FPIC_SELECT_MAX_ROWS (2^24) rows match: narrow the request"); return NULL; }
        capacity = matched;
    }
    const size_t rows = (size_t)capacity, word = dtype == FPIC_F32 ? sizeof(float) : sizeof(double);
    napi_value bi, bp, bv, out, v, ids, pos, vel;
    void *di = NULL, *dp = NULL, *dv = NULL;
    NAPI_OK(env, napi_create_arraybuffer(env, rows * sizeof(uint32_t), &di, &bi));
    NAPI_OK(env, napi_create_arraybuffer(env, 3 * rows * word, &dp, &bp));
    NAPI_OK(env, napi_create_arraybuffer(env, 3 * rows * word, &dv, &bv));
    if (fpic_select(h, &s, scope, capacity, rows ? (uint32_t*)di : NULL, rows ? dp : NULL, rows ? dv : NULL, dtype, &matched) != FPIC_OK) return throw_fpic(env, h);
    NAPI_OK(env, napi_create_object(env, &out));
    if (matched <= capacity) {
        const napi_typedarray_type real = dtype == FPIC_F32 ? napi_float32_array : napi_float64_array;
        NAPI_OK(env, napi_create_typedarray(env, napi_uint32_array, (size_t)matched, bi, 0, &ids));
        NAPI_OK(env, napi_create_typedarray(env, real, 3 * (size_t)matched, bp, 0, &pos));
        NAPI_OK(env, napi_create_typedarray(env, real, 3 * (size_t)matched, bv, 0, &vel));
    } else {
        NAPI_OK(env, napi_get_null(env, &ids));
        pos = vel = ids;
    }
    NAPI_OK(env, napi_set_named_property(env, out, "ids", ids));
    NAPI_OK(env, napi_set_named_property(env, out, "position", pos));
    NAPI_OK(env, napi_set_named_property(env, out, "velocity", vel));
    NAPI_OK(env, napi_create_double(env, (double)matched, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "matched", v));
    return out;
}

/* moments(h, species, mask, scope, out: BigInt64Array of popcount(mask) * nodes) -> { rejected, spilled }; the grids land in
 * `out` in ascending bit order.  The array's type and length are checked here, the request itself by the library. */
static napi_value n_moments(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int sp, scope; double mask;
    if (!get_args(env, info, 5, argv, &h) || !get_species(env, argv[1], &sp) || !get_double(env, argv[2], &mask) || !get_scope(env, argv[3], &scope)) return NULL;
    if (!(mask >= 1 && mask <= (double)FPIC_MOM_ORDER2) || mask != (double)(uint32_t)mask) {
        napi_throw_range_error(env, NULL, ".mask <- must be a mask of FPIC_MOM_N .. FPIC_MOM_SYZ (bits 0 .. 9), not zero");
        return NULL;
    }
    napi_typedarray_type t; void* data; size_t len;
    if (!get_typed(env, argv[4], &t, &data, &len)) return NULL;
    if (!data || t != napi_bigint64_array) { napi_throw_type_error(env, NULL, ".out <- expected a BigInt64Array"); return NULL; }
    size_t grids = 0;
    for (uint32_t m = (uint32_t)mask; m; m &= m - 1) ++grids;
    if (!check_len(env, "out", len, grids * g_box->nodes)) return NULL;
    fpic_moments_spec s;
    memset(&s, 0, sizeof s);
    s.species = sp; s.mask = (uint32_t)mask;
    fpic_moments_info mi;
    if (fpic_moments(h, &s, scope, (int64_t*)data, &mi) != FPIC_OK) return throw_fpic(env, h);
    napi_value out, v;
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_create_double(env, (double)mi.rejected, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "rejected", v));
    NAPI_OK(env, napi_create_double(env, (double)mi.spilled, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "spilled", v));
    return out;
}

/* ---- series: the field at points and the state of tracer particles as rows (fpic_series_*).  A request travels as three
 * typed arrays: points Float64Array of 3 P (metres), species Int32Array and ids Uint32Array of M each; null / undefined is an
 * empty list.  The arrays' types and lengths are checked here, the request itself by the library. */
static int get_series_request(napi_env env, napi_value* argv, fpic_series_spec* s)
{
    napi_typedarray_type tp, ts, ti; void *pp, *ps, *pi; size_t lp, ls, li;
    if (!get_typed(env, argv[0], &tp, &pp, &lp) || !get_typed(env, argv[1], &ts, &ps, &ls) || !get_typed(env, argv[2], &ti, &pi, &li)) return 0;
    if ((pp && tp != napi_float64_array) || (ps && ts != napi_int32_array) || (pi && ti != napi_uint32_array)) {
        napi_throw_type_error(env, NULL, ".points <- expected Float64Array points, Int32Array species and Uint32Array ids");
        return 0;
    }
    if (lp % 3) { napi_throw_range_error(env, NULL, ".points <- expected three numbers per point"); return 0; }
    if (!check_len(env, "species", ls, li)) return 0;
    if (lp / 3 > FPIC_SERIES_MAX_POINTS) { napi_throw_range_error(env, NULL, ".points <- more than FPIC_SERIES_MAX_POINTS (4096) points"); return 0; }
    if (li > FPIC_SERIES_MAX_TRACERS) { napi_throw_range_error(env, NULL, ".tracers <- more than FPIC_SERIES_MAX_TRACERS (65536) tracers"); return 0; }
    memset(s, 0, sizeof *s);
    s->npoints = (uint32_t)(lp / 3); s->ntracers = (uint32_t)li;
    s->points = lp ? (const double*)pp : NULL;
    s->tracer_species = li ? (const int32_t*)ps : NULL;
    s->tracer_id = li ? (const uint32_t*)pi : NULL;
    return 1;
}

static napi_value new_f64(napi_env env, size_t n, double** data)
{
    napi_value buf, arr;
    void* p = NULL;
    NAPI_OK(env, napi_create_arraybuffer(env, n * sizeof(double), &p, &buf));
    NAPI_OK(env, napi_create_typedarray(env, napi_float64_array, n, buf, 0, &arr));
    *data = (double*)p;
    return arr;
}

/* series(h, points, species, ids, scope) -> { points: Float64Array of 8 P, tracers: Float64Array of 8 M } */
static napi_value n_series(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; int scope; fpic_series_spec s;
    if (!get_args(env, info, 5, argv, &h) || !get_scope(env, argv[4], &scope) || !get_series_request(env, argv + 1, &s)) return NULL;
    double *pd = NULL, *td = NULL;
    napi_value pts = new_f64(env, (size_t)8 * s.npoints, &pd), trs = new_f64(env, (size_t)8 * s.ntracers, &td), out;
    if (!pts || !trs) return NULL;
    if (fpic_series_now(h, &s, scope, pd, td) != FPIC_OK) return throw_fpic(env, h);
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_set_named_property(env, out, "points", pts));
    NAPI_OK(env, napi_set_named_property(env, out, "tracers", trs));
    return out;
}

/* recordSeries(h, every, capacity, points, species, ids) */
static napi_value n_record_series(napi_env env, napi_callback_info info)
{
    napi_value argv[6]; fpic_handle* h; double every, cap; fpic_series_spec s;
    if (!get_args(env, info, 6, argv, &h) || !get_double(env, argv[1], &every) || !get_double(env, argv[2], &cap) || !get_series_request(env, argv + 3, &s)) return NULL;
    if (every < 0 || every > 2147483647.0 || cap < 0 || cap > 4294967295.0) { napi_throw_range_error(env, NULL, ".every <- out of range"); return NULL; }
    if (fpic_series_record(h, every > 0 ? &s : NULL, (int)every, (uint32_t)cap) != FPIC_OK) return throw_fpic(env, h);
    g_box->series_points = every > 0 ? s.npoints : 0;
    g_box->series_tracers = every > 0 ? s.ntracers : 0;
    return undefined(env);
}

/* seriesHistory(h, scope) -> { rows, dropped, substep: Float64Array of rows, points: Float64Array [rows][P][8],
 * tracers: Float64Array [rows][M][8] } (the rows recorded since the last call, oldest first) */
static napi_value n_series_history(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; int scope;
    if (!get_args(env, info, 2, argv, &h) || !get_scope(env, argv[1], &scope)) return NULL;
    uint64_t n = 0, dropped = 0;
    if (fpic_series_history(h, scope, NULL, NULL, NULL, 0, &n, &dropped) != FPIC_OK) return throw_fpic(env, h);
    double *sd = NULL, *pd = NULL, *td = NULL;
    napi_value sub = new_f64(env, (size_t)n, &sd), pts = new_f64(env, (size_t)n * 8 * g_box->series_points, &pd),
               trs = new_f64(env, (size_t)n * 8 * g_box->series_tracers, &td), out, v;
    if (!sub || !pts || !trs) return NULL;
    uint64_t* steps = (uint64_t*)calloc((size_t)n + 1, sizeof(uint64_t));
    if (!steps) { napi_throw_error(env, NULL, "host allocation failed"); return NULL; }
    if (fpic_series_history(h, scope, steps, pd, td, n, &n, &dropped) != FPIC_OK) { free(steps); return throw_fpic(env, h); }
    for (uint64_t i = 0; i < n; ++i) sd[i] = (double)steps[i];
    free(steps);
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_create_double(env, (double)n, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "rows", v));
    NAPI_OK(env, napi_create_double(env, (double)dropped, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "dropped", v));
    NAPI_OK(env, napi_set_named_property(env, out, "substep", sub));
    NAPI_OK(env, napi_set_named_property(env, out, "points", pts));
    NAPI_OK(env, napi_set_named_property(env, out, "tracers", trs));
    return out;
}

/* ---- modes: the Fourier amplitudes of the node fields at chosen wave vectors (fpic_modes_*).  A request travels as an
 * Int32Array of 3 M wave-vector components and the mask of quantities.  The array's type and length are checked here, the
 * request itself by the library. */
static int get_modes_request(napi_env env, napi_value* argv, fpic_modes_spec* s, size_t* width)
{
    napi_typedarray_type tm; void* pm; size_t lm; double mask;
    if (!get_typed(env, argv[0], &tm, &pm, &lm) || !get_double(env, argv[1], &mask)) return 0;
    if (pm && tm != napi_int32_array) { napi_throw_type_error(env, NULL, ".modes <- expected an Int32Array of wave-vector components"); return 0; }
    if (lm % 3) { napi_throw_range_error(env, NULL, ".modes <- expected three components per wave vector"); return 0; }
    if (lm / 3 > FPIC_MODES_MAX) { napi_throw_range_error(env, NULL, ".nmodes <- must lie in [1, FPIC_MODES_MAX (256)]"); return 0; }
    if (mask < 0 || mask > 4294967295.0 || mask != (double)(uint32_t)mask) { napi_throw_range_error(env, NULL, ".mask <- expected a mask of quantity bits"); return 0; }
    memset(s, 0, sizeof *s);
    s->nmodes = (uint32_t)(lm / 3); s->mask = (uint32_t)mask;
    s->modes = lm ? (const int32_t*)pm : NULL;
    size_t nq = 0;
    for (uint32_t b = s->mask & FPIC_MODE_ALL; b; b >>= 1) nq += b & 1u;
    *width = 2 * (size_t)s->nmodes * nq;
    return 1;
}

/* modes(h, modes, mask, scope) -> Float64Array [M][nq][2] (re, im; the quantities in ascending bit order) */
static napi_value n_modes(napi_env env, napi_callback_info info)
{
    napi_value argv[4]; fpic_handle* h; int scope; fpic_modes_spec s; size_t width;
    if (!get_args(env, info, 4, argv, &h) || !get_scope(env, argv[3], &scope) || !get_modes_request(env, argv + 1, &s, &width)) return NULL;
    double* d = NULL;
    napi_value out = new_f64(env, width ? width : 2, &d);      /* (a refused request writes nothing) */
    if (!out) return NULL;
    if (fpic_modes_now(h, &s, scope, d) != FPIC_OK) return throw_fpic(env, h);
    return out;
}

/* recordModes(h, every, capacity, modes, mask) */
static napi_value n_record_modes(napi_env env, napi_callback_info info)
{
    napi_value argv[5]; fpic_handle* h; double every, cap; fpic_modes_spec s; size_t width;
    if (!get_args(env, info, 5, argv, &h) || !get_double(env, argv[1], &every) || !get_double(env, argv[2], &cap) || !get_modes_request(env, argv + 3, &s, &width)) return NULL;
    if (every < 0 || every > 2147483647.0 || cap < 0 || cap > 4294967295.0) { napi_throw_range_error(env, NULL, ".every <- out of range"); return NULL; }
    if (fpic_modes_record(h, every > 0 ? &s : NULL, (int)every, (uint32_t)cap) != FPIC_OK) return throw_fpic(env, h);
    g_box->modes_width = every > 0 ? width : 0;
    return undefined(env);
}

/* modesHistory(h, scope) -> { rows, dropped, substep: Float64Array of rows, values: Float64Array [rows][M][nq][2] } (the rows
 * recorded since the last call, oldest first) */
static napi_value n_modes_history(napi_env env, napi_callback_info info)
{
    napi_value argv[2]; fpic_handle* h; int scope;
    if (!get_args(env, info, 2, argv, &h) || !get_scope(env, argv[1], &scope)) return NULL;
    uint64_t n = 0, dropped = 0;
    if (fpic_modes_history(h, scope, NULL, NULL, 0, &n, &dropped) != FPIC_OK) return throw_fpic(env, h);
    double *sd = NULL, *vd = NULL;
    napi_value sub = new_f64(env, (size_t)n, &sd), vals = new_f64(env, (size_t)n * g_box->modes_width, &vd), out, v;
    if (!sub || !vals) return NULL;
    uint64_t* steps = (uint64_t*)calloc((size_t)n + 1, sizeof(uint64_t));
    if (!steps) { napi_throw_error(env, NULL, "host allocation failed"); return NULL; }
    if (fpic_modes_history(h, scope, steps, vd, n, &n, &dropped) != FPIC_OK) { free(steps); return throw_fpic(env, h); }
    for (uint64_t i = 0; i < n; ++i) sd[i] = (double)steps[i];
    free(steps);
    NAPI_OK(env, napi_create_object(env, &out));
    NAPI_OK(env, napi_create_double(env, (double)n, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "rows", v));
    NAPI_OK(env, napi_create_double(env, (double)dropped, &v));
    NAPI_OK(env, napi_set_named_property(env, out, "dropped", v));
    NAPI_OK(env, napi_set_named_property(env, out, "substep", sub));
    NAPI_OK(env, napi_set_named_property(env, out, "values", vals));
    return out;
}

static napi_value n_build_arch(napi_env env, napi_callback_info info)
{
    (void)info;
    napi_value s;
    NAPI_OK(env, napi_create_string_utf8(env, fpic_build_arch(), NAPI_AUTO_LENGTH, &s));
    return s;
}

int fusionsor_register(napi_env env, napi_value exports); /* fusionsor_napi.c */

static napi_value init(napi_env env, napi_value exports)
{
    struct { const char* name; napi_callback fn; } table[] = {
        { "create", n_create }, { "destroy", n_destroy }, { "setParticles", n_set_particles },
        { "setGrid", n_set_grid }, { "setRandomState", n_set_random_state }, { "addCurrentLoop", n_add_current_loop },
        { "addCurrentZ", n_add_current_z }, { "addBZ", n_add_bz }, { "addBTheta", n_add_btheta },
        { "precalc", n_precalc }, { "step", n_step }, { "substeps", n_substeps }, { "stepAsync", n_step_async }, { "density", n_density }, { "deposit", n_deposit },
        { "densityFinish", n_density_finish }, { "readGrid", n_read_grid }, { "getParticles", n_get_particles },
        { "getCells", n_get_cells }, { "sort", n_sort }, { "sync", n_sync }, { "profile", n_profile },
        { "getStats", n_get_stats }, { "saveCheckpoint", n_save_checkpoint }, { "loadCheckpoint", n_load_checkpoint }, { "resetStats", n_reset_stats }, { "buildArch", n_build_arch },
        { "addSpecies", n_add_species }, { "setParticlesRange", n_set_particles_range }, { "getParticlesOf", n_get_particles_of },
        { "getCellsOf", n_get_cells_of }, { "getParticlesRange", n_get_particles_range }, { "commInfo", n_comm_info }, { "addB", n_add_b }, { "setField3", n_set_field3 }, { "readField3", n_read_field3 },
        { "commUniqueId", n_comm_unique_id }, { "commInit", n_comm_init }, { "commDestroy", n_comm_destroy },
        { "domainInit", n_domain_init }, { "domainSetParticles", n_domain_set_particles }, { "domainGetParticles", n_domain_get_particles },
        { "domainStats", n_domain_stats },
        { "energy", n_energy }, { "recordEnergy", n_record_energy }, { "energyHistory", n_energy_history },
        { "histogram", n_histogram }, { "select", n_select }, { "load", n_load }, { "collide", n_collide }, { "collideEvery", n_collide_every }, { "collisionStats", n_collision_stats }, { "clearCollisions", n_clear_collisions },
        { "force", n_force }, { "forceOn", n_force_on }, { "forceStats", n_force_stats }, { "clearForces", n_clear_forces },
        { "collideGas", n_collide_gas }, { "collideGasEvery", n_collide_gas_every }, { "gasStats", n_gas_stats }, { "clearGas", n_clear_gas },
        { "remove", n_remove }, { "removeEvery", n_remove_every }, { "removeStats", n_remove_stats }, { "clearRemovals", n_clear_removals }, { "renumber", n_renumber },
        { "inject", n_inject }, { "injectEvery", n_inject_every }, { "injectStats", n_inject_stats }, { "clearInjections", n_clear_injections },
        { "reserve", n_reserve }, { "population", n_population },
        { "ionize", n_ionize }, { "ionizeEvery", n_ionize_every }, { "ionizeStats", n_ionize_stats }, { "clearIonization", n_clear_ionization },
        { "burn", n_burn }, { "burnEvery", n_burn_every }, { "burnStats", n_burn_stats }, { "clearBurn", n_clear_burn },
        { "collidePair", n_collide_pair }, { "collidePairEvery", n_collide_pair_every }, { "pairStats", n_pair_stats }, { "clearPairs", n_clear_pairs },
        { "fusionYield", n_fusion_yield }, { "fusionYieldEvery", n_fusion_yield_every }, { "fusionStats", n_fusion_stats }, { "fusionGrid", n_fusion_grid }, { "clearFusion", n_clear_fusion },
        { "fusionSpectrum", n_fusion_spectrum }, { "fusionSpectrumEvery", n_fusion_spectrum_every }, { "fusionSpectrumRead", n_fusion_spectrum_read }, { "clearFusionSpectra", n_clear_fusion_spectra },
        { "moments", n_moments },
        { "series", n_series }, { "recordSeries", n_record_series }, { "seriesHistory", n_series_history },
        { "modes", n_modes }, { "recordModes", n_record_modes }, { "modesHistory", n_modes_history },
    };
    for (size_t i = 0; i < sizeof table / sizeof table[0]; ++i) {
        napi_value fn;
        if (napi_create_function(env, table[i].name, NAPI_AUTO_LENGTH, table[i].fn, NULL, &fn) != napi_ok ||
            napi_set_named_property(env, exports, table[i].name, fn) != napi_ok) {
            napi_throw_error(env, NULL, "addon initialisation failed");
            return NULL;
        }
    }
    if (!fusionsor_register(env, exports)) {
        napi_throw_error(env, NULL, "addon initialisation failed");
        return NULL;
    }
    return exports;
}

#ifndef NODE_GYP_MODULE_NAME
#define NODE_GYP_MODULE_NAME fusionpic_napi
#endif
NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
