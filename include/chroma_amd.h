/* chroma_amd.h -- C ABI of the MI355X-native Chroma propagator (libchroma_amd.so).
 *
 * Every entry point replaces one thing the reference binds through PyCUDA
 * (a JIT-compiled `extern "C" __global__` kernel launched from Python, or a
 * make_gpu_struct() upload).  The "replaces" line on each declaration cites the
 * reference interface (paths relative to youngsm/chroma-lite).
 *
 * Conventions
 *  - plain C types only; no torch / HIP types in the signatures.  `stream` is a
 *    hipStream_t passed as void* (NULL = default stream).
 *  - pointers named d_* are DEVICE pointers (e.g. torch.Tensor.data_ptr()),
 *    pointers named h_* are host pointers.
 *  - photon vectors (pos/dir/pol) are float3-packed: 3 floats per photon,
 *    exactly the reference's ga.vec.float3 arrays (chroma/gpu/photon.py:46-48).
 *  - every function returns 0 on success or a nonzero chr_status; the message
 *    of the last failure on the calling thread is chr_last_error().
 *  - all launches are asynchronous on `stream` unless documented otherwise;
 *    functions that return a count to the host synchronise the stream.
 */
#ifndef CHROMA_AMD_H
#define CHROMA_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

enum chr_status {
    CHR_OK = 0,
    CHR_ERR_INVALID = 1,     /* bad argument (reference: ValueError / assert) */
    CHR_ERR_HIP = 2,         /* HIP runtime error (reference: pycuda LogicError/LaunchError) */
    CHR_ERR_NOMEM = 3,
    CHR_ERR_STACK = 4,       /* BVH stack overflow (reference: printf in mesh.h:111-114) */
    CHR_ERR_INTERNAL = 5     /* a device-side consistency check failed (no reference counterpart) */
};

/* photon history bits as stored on the device (reference photon.h:53-68).
 * NOTE the reference keeps history in an unsigned short on the device, so
 * NAN_ABORT is bit 15 there (and any propagate clears bits 16..31). */
enum chr_history {
    CHR_NO_HIT = 1u << 0, CHR_BULK_ABSORB = 1u << 1, CHR_SURFACE_DETECT = 1u << 2,
    CHR_SURFACE_ABSORB = 1u << 3, CHR_RAYLEIGH_SCATTER = 1u << 4, CHR_REFLECT_DIFFUSE = 1u << 5,
    CHR_REFLECT_SPECULAR = 1u << 6, CHR_SURFACE_REEMIT = 1u << 7, CHR_SURFACE_TRANSMIT = 1u << 8,
    CHR_BULK_REEMIT = 1u << 9, CHR_CHERENKOV = 1u << 10, CHR_SCINTILLATION = 1u << 11,
    CHR_NAN_ABORT = 1u << 15
};

/* surface models (reference geometry_types.h:22) */
enum chr_surface_model { CHR_SURFACE_DEFAULT = 0, CHR_SURFACE_COMPLEX = 1, CHR_SURFACE_WLS = 2,
                         CHR_SURFACE_DICHROIC = 3, CHR_SURFACE_ANGULAR = 4 };

/* ---------------------------------------------------------------- geometry
 * Host-side description of a flattened, BVH-indexed geometry.  All tables are
 * sampled on one wavelength grid (wavelength_start + i*wavelength_step,
 * i < wavelength_n) and one time grid, as GPUGeometry does
 * (chroma/gpu/geometry.py:44-107).  EVERY table pointer must address n+1
 * floats: the last element duplicates element n-1 (the reference's
 * interp_property reads fp[n] at x == last grid point, geometry.h:61-74).
 */
typedef struct chr_material_desc {         /* reference struct Material, geometry_types.h:4-20 */
    uint32_t num_comp;
    const float *refractive_index;          /* [wavelength_n+1] */
    const float *absorption_length;
    const float *scattering_length;
    const float *comp_reemission_prob;      /* [num_comp][wavelength_n+1] */
    const float *comp_reemission_wvl_cdf;   /* [num_comp][wavelength_n+1] */
    const float *comp_reemission_time_cdf;  /* [num_comp][time_n+1] */
    const float *comp_absorption_length;    /* [num_comp][wavelength_n+1] */
} chr_material_desc;

typedef struct chr_surface_desc {          /* reference struct Surface, geometry_types.h:60-79 */
    int32_t present;                        /* 0: NULL slot (the `None` surface) */
    uint32_t model;                         /* chr_surface_model */
    uint32_t transmissive;
    float thickness;
    const float *detect, *absorb, *reemit, *reflect_diffuse, *reflect_specular,
                *eta, *k, *reemission_cdf;  /* [wavelength_n+1] each */
    uint32_t dichroic_nangles;              /* 0: no DichroicProps */
    const float *dichroic_angles;           /* [nangles] */
    const float *dichroic_reflect;          /* [nangles][wavelength_n+1] */
    const float *dichroic_transmit;         /* [nangles][wavelength_n+1] */
    uint32_t angular_nangles;               /* 0: no AngularProps */
    const float *angular_angles, *angular_transmit, *angular_reflect_specular,
                *angular_reflect_diffuse;   /* [nangles] */
} chr_surface_desc;

typedef struct chr_wireplane_desc {        /* reference struct WirePlane, geometry_types.h:42-58 */
    float origin[3], u[3], v[3];
    float pitch, radius, umin, umax, vmin, vmax, v0;
    int32_t surface_index, material_outer_index, material_inner_index;
    uint32_t color;
} chr_wireplane_desc;

typedef struct chr_geometry_desc {         /* reference struct Geometry, geometry_types.h:124-139 */
    uint32_t nvertices, ntriangles, nnodes;
    uint32_t nmaterials, nsurfaces, nwireplanes;
    const float *h_vertices;                /* [nvertices*3] */
    const uint32_t *h_triangles;            /* [ntriangles*3] */
    const uint32_t *h_material_codes;       /* [ntriangles]: m1<<24 | m2<<16 | surf<<8 (gpu/geometry.py:401-404) */
    const uint32_t *h_nodes;                /* [nnodes*4] packed uint4 BVH nodes (bvh/bvh.py:106-195) */
    float world_origin[3];
    float world_scale;
    uint32_t wavelength_n; float wavelength_start, wavelength_step;
    uint32_t time_n; float time_start, time_step;
    const chr_material_desc *materials;
    const chr_surface_desc *surfaces;
    const chr_wireplane_desc *wireplanes;
} chr_geometry_desc;

typedef struct chr_geometry chr_geometry;  /* opaque device-resident geometry */

/* replaces: GPUGeometry.__init__ device uploads (chroma/gpu/geometry.py:14-526).
 * Copies everything to HBM of the current device, builds the traversal layout.
 * Synchronous. */
int chr_geometry_create(const chr_geometry_desc *desc, chr_geometry **out);
int chr_geometry_destroy(chr_geometry *g);
/* bytes of HBM held by the geometry (reference: GPUGeometry.device_usage_str) */
int chr_geometry_device_bytes(const chr_geometry *g, uint64_t *bytes);
/* words (4 B) of the physics tables and records: the hot part the step kernels
 * copy to LDS when it fits (property tables, identical tables stored once, the
 * material / surface records) and the whole (+ re-emission time CDFs and their
 * bucket indexes, read from HBM).  No reference counterpart (diagnostic). */
int chr_geometry_phys_words(const chr_geometry *g, uint32_t *hot_words, uint32_t *total_words);

/* ----------------------------------------------------------------- photons */
typedef struct chr_photons {               /* reference GPUPhotons arrays, photon.py:46-62 */
    float *d_pos, *d_dir, *d_pol;          /* float3-packed [n*3] */
    float *d_wavelengths, *d_t, *d_weights;
    uint32_t *d_flags;
    int32_t *d_last_hit_triangles;
    uint32_t *d_evidx;
} chr_photons;

/* ---------------------------------------------------------------- random */
/* RNG slot states: 6 x u32 per slot, SoA (word k of slot s at d_states[k*nslots+s]).
 * replaces: get_rng_states / init_rng (chroma/gpu/tools.py:117-145):
 * curand_init(seed, subsequence = slot, offset) for every slot. */
int chr_init_rng(uint32_t *d_states, uint32_t nslots, uint64_t seed, uint64_t offset, void *stream);
/* extension for photon-sharded runs: slot s = curand_init(seed, first_subsequence + s, offset)
 * (first_subsequence + nslots <= 2^32); chr_init_rng is first_subsequence = 0. */
int chr_init_rng_subseq(uint32_t *d_states, uint32_t nslots, uint64_t seed, uint64_t first_subsequence,
                        uint64_t offset, void *stream);
/* copy slot states to the host (tests; 6*nslots words, SoA) */
int chr_rng_download(const uint32_t *d_states, uint32_t nslots, uint32_t *h_out, void *stream);

/* ---------------------------------------------------------------- gensteps
 * A genstep is "a charged particle made nphotons photons along this segment":
 * the compact record a particle simulation writes (Opticks' term) and the
 * device turns into photons.  replaces: the reference's Geant4 light source
 * (chroma/generator/, bin/chroma-sim), which needs a host particle simulation
 * per photon; here the caller supplies the yield (nphotons) and the device
 * draws the photons.  64 bytes, 16 words.
 *
 * Photons are numbered step-major (photon k of the call belongs to the step i
 * with offset[i] <= k < offset[i+1], offset = exclusive prefix sum of
 * nphotons).  Photon k is drawn by RNG slot k mod rng_nslots; a slot draws its
 * photons in ascending k, so the result depends on the slot states, rng_nslots
 * and the records only.  Draw order of one photon (csrc/genstep.h), every
 * multiply-add an explicit fmaf:
 *   f = uniform01
 *   pos = fma(f, dx, x0) per component, t = fma(f, dt, t0)
 *   weight = 1, last_hit = -1, evidx = the record's
 *   CHR_GEN_ISOTROPIC:     dir = uniform_sphere (2 draws); a = uniform_sphere (2 draws),
 *                          pol = cross(a, dir) / |cross(a, dir)|;
 *                          wavelength = wl_lo + uniform01 * (wl_hi - wl_lo); flags = 0
 *   CHR_GEN_SCINTILLATION: wavelength = sample_cdf(material's comp_reemission_wvl_cdf[component]) (1 draw);
 *                          t += sample_cdf(comp_reemission_time_cdf[component]) (1 draw);
 *                          dir, pol as ISOTROPIC (4 draws); flags = CHR_SCINTILLATION
 *   CHR_GEN_CHERENKOV:     u = dx / |dx|; at most CHR_GEN_MAX_TRIES times:
 *                            1/wl = 1/wl_hi + uniform01 * (1/wl_lo - 1/wl_hi), n = refractive_index(wl)
 *                            (the propagate kernels' interp_property), c = 1 / (beta * n),
 *                            accept when 1 - c*c > uniform01 * s2max, s2max = 1 - 1/(beta * n_max)^2
 *                            with n_max the largest n over [wl_lo, wl_hi];
 *                          tries used up: wl = the wavelength of n_max (counted in *exhausted);
 *                          phi = uniform01 * 2 pi (1 draw); s = sqrt(1 - c*c);
 *                          (e1, e2): a = the coordinate axis of u's smallest |component| (x before y
 *                          before z on ties), e1 = cross(u, a) / |cross(u, a)|, e2 = cross(u, e1);
 *                          w = cos(phi) e1 + sin(phi) e2; dir = c u + s w;
 *                          pol = normalise(c dir - u), evaluated as normalise(c w - s u) (the same
 *                          vector divided by s, without the cancellation); flags = CHR_CHERENKOV */
enum chr_genstep_kind { CHR_GEN_ISOTROPIC = 0, CHR_GEN_SCINTILLATION = 1, CHR_GEN_CHERENKOV = 2 };
#define CHR_GEN_MAX_TRIES 1024
typedef struct chr_genstep {
    uint32_t kind, nphotons, material, evidx;   /* chr_genstep_kind; material: index into the geometry's */
    float x0[3], t0;                             /* start of the segment (mm, ns) */
    float dx[3], dt;                             /* its extent: photons start at x0 + f dx, t0 + f dt */
    float wl_lo, wl_hi, beta;                    /* wavelength range (nm; ISOTROPIC, CHERENKOV); v/c (CHERENKOV) */
    uint32_t component;                          /* scintillation component (SCINTILLATION) */
} chr_genstep;

/* *total = sum of nphotons (64-bit: may exceed what one call generates) */
int chr_gensteps_count(const chr_genstep *h_steps, uint32_t nsteps, uint64_t *total);
/* Generate the steps' photons into out[first_photon, first_photon + total) (arrays of >= capacity
 * photons; first_photon + total <= capacity) with the slot states d_rng_states, which are advanced.
 * All nine fields are written.  Every record is validated on the host before any launch
 * (CHR_ERR_INVALID: unknown kind, material >= nmaterials, SCINTILLATION component >= num_comp,
 * a non-finite field, wl_lo > wl_hi or a non-positive limit, CHERENKOV with |dx| = 0, beta outside
 * (0, 1] or beta * n_max <= 1, total > capacity - first_photon or > 2^31 - 1, rng_nslots = 0).
 * *ngenerated = total, *exhausted = photons whose rejection loop ran out.  Synchronous. */
int chr_generate_photons(const chr_geometry *g, const chr_genstep *h_steps, uint32_t nsteps,
                         const chr_photons *out, uint32_t first_photon, uint32_t capacity,
                         uint32_t *d_rng_states, uint32_t rng_nslots, uint32_t *ngenerated,
                         uint32_t *exhausted, void *stream);
/* The same on the host (no GPU needed), over a geometry descriptor: out holds HOST arrays of
 * >= first_photon + total photons, h_rng_states host slot states in the device's SoA layout.
 * Bit-identical to chr_generate_photons (one source, csrc/genstep.h). */
int chr_generate_photons_host(const chr_geometry_desc *desc, const chr_genstep *h_steps, uint32_t nsteps,
                              const chr_photons *out, uint32_t first_photon, uint32_t capacity,
                              uint32_t *h_rng_states, uint32_t rng_nslots, uint32_t *ngenerated,
                              uint32_t *exhausted);
/* chr_init_rng_subseq on the host: the same states in the same SoA layout */
int chr_init_rng_host(uint32_t *h_states, uint32_t nslots, uint64_t seed, uint64_t first_subsequence,
                      uint64_t offset);

/* -------------------------------------------------------------- propagate */
/* replaces: the `propagate` kernel (chroma/cuda/propagate.cu:254-366), one
 * chunk launch: slots [0, nthreads), photon = d_input_queue[first_photon + slot].
 * Survivors are appended to d_output_queue in input order (stable; the
 * reference's warp-atomic order is nondeterministic) and d_output_queue[0]
 * counts them (+1, photon.py:248-250).  d_scratch must hold
 * chr_propagate_scratch_words(nthreads) u32 words. */
uint64_t chr_propagate_scratch_words(uint32_t nthreads);
int chr_propagate_chunk(const chr_geometry *g, const chr_photons *ph, uint32_t *d_rng_states,
                        uint32_t rng_nslots, int32_t first_photon, int32_t nthreads,
                        const uint32_t *d_input_queue, uint32_t *d_output_queue,
                        int32_t max_steps, int32_t use_weights, int32_t scatter_first,
                        uint32_t *d_scratch, void *stream);

typedef struct chr_propagate_stats {
    uint32_t steps_run;         /* host-loop steps executed */
    uint32_t launches;          /* chunk launches */
    uint32_t final_alive;       /* photons still in the queue at exit */
    uint32_t stack_overflows;   /* traversals that exceeded the 1000-entry stack */
    double kernel_ms;           /* summed device time of the propagate kernels (HIP events; device-driven
                                   propagates record them only with CHR_SLOT_TIMING=1, else 0) */
    uint64_t nodes_visited;     /* BVH nodes / triangles / walks: filled only by the counting */
    uint64_t triangles_tested;  /* kernel variant (CHR_PROPAGATE_VARIANT=5), zero otherwise */
    uint64_t traversals;
    uint64_t wave_node_steps;     /* node / triangle steps executed per wave (SIMD efficiency = */
    uint64_t wave_triangle_steps; /* nodes_visited / (64 * wave_node_steps)); counting variant only */
    uint64_t wave_fill_cycles;    /* s_memtime cycles waves spent in fill_state (traversal) and in */
    uint64_t wave_step_cycles;    /* whole photon step loops; counting variant only */
    double trace_ms;              /* device time of the BVH-walk kernel (trace_kernel) alone, HIP events */
    uint32_t trace_launches;      /* one-step launches walked by trace_kernel */
    uint32_t live_record_slots;   /* one-step slots whose shade_kernel read live records (CHR_LIVE_RECORDS) */
    uint64_t trace_rays;          /* queued photons handed to those launches */
    uint32_t trace_ms_n;          /* entries of trace_launch_ms filled (first CHR_TRACE_MS_MAX launches) */
    float trace_launch_ms[32];    /* device time of each trace_kernel launch, in order */
    uint32_t flat_walks;          /* walks with a direction component of non-finite reciprocal (the reference's
                                     slab test then skips that axis) done by trace_kernel (flat-axis slab test) */
    uint32_t flat_walks_whole;    /* such walks done by the multi-step (tail) kernel */
    uint32_t tail_photons;        /* photons handed to the multi-step (tail) launch (nsteps policy) */
    double tail_ms;               /* device time of that launch (HIP events; CHR_SLOT_TIMING=1, else 0) */
    uint32_t tail_max_steps;      /* most steps one photon ran in the tail launch */
    uint32_t tail_slowest_steps;  /* steps of the photon that took longest in the tail launch */
    uint64_t tail_max_cycles;     /* that photon's time in ticks of the 100 MHz s_memrealtime clock */
    uint32_t tail_long_photons;   /* photons of > 64 steps in the tail launch, and summed over them: */
    uint32_t reserved2;
    uint64_t tail_long_steps;     /*   steps, */
    uint64_t tail_long_ticks;     /*   100 MHz ticks from load to write-back, */
    uint64_t tail_long_walk_ticks;        /*   ticks in the BVH walk (wave-adaptive tail kernel), */
    uint64_t tail_long_walk_iterations;   /*   and dependent walk iterations */
    uint32_t host_syncs;          /* waits that drain the stream (the host reads the survivor count): one
                                     per host step when host-driven, 1 when the steps are device-driven */
    uint32_t tail_long_paired_steps;  /* the long photons' steps whose walk had a tester wave (walk_pair) */
    uint32_t trace_launch_rays[32];   /* queued photons of each trace_kernel launch, in order */
} chr_propagate_stats;
#define CHR_TRACE_MS_MAX 32

/* Resources of the kernels on the default propagate path, from the code object
 * (hipFuncGetAttributes): which = 0 trace_kernel (BVH walk of one-step launches),
 * 1 shade_kernel, 2 the tail's group-walk kernel, 3 the fused step kernel.
 * No reference counterpart (bench diagnostics). */
typedef struct chr_kernel_attr {
    uint64_t private_bytes;     /* scratch per work-item (0: no private segment) */
    uint64_t lds_bytes;         /* static LDS per workgroup */
    int32_t vgprs;              /* architected VGPRs per work-item */
    int32_t max_threads;        /* max workgroup size */
    char name[96];
} chr_kernel_attr;
int chr_kernel_info(int32_t which, chr_kernel_attr *out);
/* Diagnostic (no reference counterpart): the tail's lone-photon walk timed in
 * isolation, walker 0 = walk_lone on one wave, 1 = the pair walk (one wave walks,
 * a second wave of the workgroup tests the triangles), 2 = the pair walk with a
 * 2-poll handshake budget, so handshakes are lost and the tail kernel's recovery
 * (the walk again with walk_lone, no more pairing in that workgroup) runs; each
 * lost handshake adds 1 << 20 to the last word; 3 = walk_up from an arbitrary
 * node (ray r: (r * 2654435761) mod nodes), 4 = walk_up from the leaf node of a
 * given record (d_rays then n x 8 words: + the record index), 5 = the grouped
 * walk's climb (one 64-lane segment) from walker 3's start, 7 = walker 3 with the
 * start node's ancestors read beforehand (the tail's prefetch).  nwaves workgroups; workgroup
 * w walks rays w, w + nwaves, ... each reps times in a row.  d_rays: n x 7 floats
 * (origin, direction, last hit triangle id as int bits); d_out: n x reps x 4 words
 * (record index or -1, iterations, 100 MHz ticks, shader-clock cycles of the walk)
 * + 1 word, the stack overflows (low 20 bits, must read 0) + lost handshakes << 20. */
int chr_walk_lone_timing(const chr_geometry *g, const float *d_rays, uint32_t n, uint32_t reps,
                         uint32_t nwaves, int32_t walker, uint32_t *d_out, void *stream);

/* replaces: GPUPhotons.propagate host loop (chroma/gpu/photon.py:226-293) for
 * track=False: queue setup (clones interleaved, 242-250), the nsteps policy
 * (261-264), chunk_iterator chunking (tools.py:159-180), queue swap and the
 * per-step survivor count (277-286).  Synchronous. */
int chr_propagate(const chr_geometry *g, const chr_photons *ph, uint32_t nphotons,
                  uint32_t true_nphotons, uint32_t ncopies,
                  uint32_t *d_rng_states, uint32_t rng_nslots,
                  int32_t nthreads_per_block, int32_t max_blocks, int32_t max_steps,
                  int32_t use_weights, int32_t scatter_first,
                  chr_propagate_stats *stats, void *stream);

/* replaces: a sequence of GPUPhotons.propagate calls sharing one rng_states
 * (the event loop of Simulation.simulate, chroma/sim.py:116-160, one propagate
 * per event): batch i = photons phs[i] (nphotons[i] = true_nphotons[i] *
 * ncopies[i]), propagated in order with the same RNG slot states and the same
 * launch shape.  Results (photons, RNG states) are bit-identical to nbatch
 * chr_propagate calls; the multi-step tail of batch i runs on a second stream
 * while batch i+1 queues, bins and walks its first step (which needs no RNG),
 * and batch i+1's first RNG use waits for that tail.  stats: nbatch entries
 * (or NULL).  Batches whose photon arrays overlap are serialised.  Synchronous. */
int chr_propagate_batches(const chr_geometry *g, const chr_photons *phs, const uint32_t *nphotons,
                          const uint32_t *true_nphotons, const uint32_t *ncopies, uint32_t nbatch,
                          uint32_t *d_rng_states, uint32_t rng_nslots,
                          int32_t nthreads_per_block, int32_t max_blocks, int32_t max_steps,
                          int32_t use_weights, int32_t scatter_first,
                          chr_propagate_stats *stats, void *stream);

/* ---------------------------------------------------------- photon tracks
 * replaces: GPUPhotons.propagate(track=True) (chroma/gpu/photon.py:252-293): the
 * host step loop with every step a single step, the copy_queue gather and the
 * per-step downloads of step_photon_ids / step_photons.  The tracks stay on the
 * device behind an opaque handle that owns its memory, in two orders.
 *
 * Track record: CHR_TRACK_WORDS u32 words, 64-byte aligned --
 *   [0] photon id   [1] history (the u32 the flags array holds)
 *   [2..4] pos   [5..7] dir   [8..10] pol   [11] wavelength   [12] t   [13] weight
 *   [14] last-hit triangle (i32)   [15] entry index k
 * Entry 0 is the input state of every photon of the first queue (the interleaved
 * clone ids of ncopies > 1 included, photon.py:242-247); entry k the state after
 * k steps of the photons queued into step k, in queue order.  evidx is not
 * stored: it is d_evidx[id].
 *   order 0, step-major:   entry 0's records, entry 1's, ...; offsets[nentries + 1]
 *   order 1, photon-major: photon 0's records by entry, photon 1's, ...;
 *                          offsets[nphotons + 1] (a photon queued at step k was
 *                          queued at every earlier step: its j-th record is entry j)
 *
 * chr_propagate_tracked is chr_propagate's host loop with one step per launch on
 * every step (never the multi-step tail, never live records or device-driven
 * slots; scatter_first on the first step only): where a step is one launch for
 * chr_propagate (a slot count that is a multiple of 64) it is the split trace +
 * shade launch here too, otherwise the chunk launches of chr_propagate_chunk.
 * The RNG slot of a photon is its position in the step's chunk on every path,
 * so photons, RNG states and records are those of the chunk loop driven from
 * the host (photon.py:252-293), word for word.  The loop ends at max_steps or
 * when the queue empties (photon.py:285-286); nentries = steps run + 1;
 * max_steps == 0 records entry 0 and launches no step; nphotons == 0 gives a
 * handle with one empty entry and launches nothing (the photon arrays' addresses
 * may then be NULL).  The step-major buffer grows
 * geometrically from capacity_hint records (0: nphotons x min(max_steps + 1, 2),
 * what entries 0 and 1 take), never nphotons x (max_steps + 1) up front.
 * CHR_ERR_INVALID before any launch for what chr_propagate refuses and a NULL out;
 * CHR_ERR_NOMEM when a buffer cannot be allocated, CHR_ERR_INTERNAL when a queue
 * word is not a photon of the call (counted on the device, never followed): then
 * everything the call allocated is freed and *out is NULL.  stats as
 * chr_propagate fills them; host_syncs <= steps run + 1.  Synchronous. */
#define CHR_TRACK_WORDS 16
typedef struct chr_tracks chr_tracks;   /* opaque, owns its device memory */
int chr_propagate_tracked(const chr_geometry *g, const chr_photons *ph, uint32_t nphotons,
                          uint32_t true_nphotons, uint32_t ncopies,
                          uint32_t *d_rng_states, uint32_t rng_nslots,
                          int32_t nthreads_per_block, int32_t max_blocks, int32_t max_steps,
                          int32_t use_weights, int32_t scatter_first,
                          uint64_t capacity_hint /* records; 0 = default */,
                          chr_tracks **out, chr_propagate_stats *stats, void *stream);
/* replaces: len(step_photon_ids) and the sum of its arrays' lengths (photon.py:252-293) */
int chr_tracks_info(const chr_tracks *t, uint32_t *nentries, uint64_t *nrecords, uint32_t *nphotons);
/* replaces: the lengths of step_photon_ids' arrays (photon.py:252-293) */
int chr_tracks_entry_counts(const chr_tracks *t, uint64_t *h_counts /*[nentries]*/);
/* the device buffers of one order (no reference counterpart, photon.py:252-293 keeps
 * none): valid until chr_tracks_free; NULL records for an empty buffer */
int chr_tracks_device(const chr_tracks *t, int32_t order /*0 step-major, 1 photon-major*/,
                      const uint32_t **d_records, const uint64_t **d_offsets);
/* replaces: the downloads of photon.py:252-293 (one .get() per array and step) with one
 * copy: h_records[nrecords * CHR_TRACK_WORDS], h_offsets[nentries + 1 or nphotons + 1];
 * either may be NULL */
int chr_tracks_copy(const chr_tracks *t, int32_t order, uint32_t *h_records, uint64_t *h_offsets);
/* NULL is accepted (as chr_bvh_result_free) */
int chr_tracks_free(chr_tracks *t);
/* replaces: the host arrays photon.py:252-293 gets from one .get() per array and step.
 * Host only: record r of h_records (as chr_tracks_copy gives them, either order) goes to
 * element r of the nine HOST arrays of h_out (nrecords photons) and its id to h_ids[r];
 * evidx[r] = h_evidx[id] (h_evidx: nphotons words).  One pass, on the library's host
 * threads.  CHR_ERR_INVALID for a NULL argument or an id >= nphotons (never followed). */
int chr_tracks_unpack(const uint32_t *h_records, uint64_t nrecords, const uint32_t *h_evidx,
                      uint32_t nphotons, const chr_photons *h_out, uint32_t *h_ids);

/* ------------------------------------------------------------ selection */
/* replaces: count_photon_hits + copy_photon_hits (propagate.cu:172-251),
 * driven by GPUPhotons.get_flat_hits (photon.py:141-209).  Hits are compacted
 * in ascending photon order.  Pass d_out.* = NULL to only count.  *nhits is
 * written on the host (synchronises). */
int chr_photon_hits(const chr_photons *ph, int32_t start_photon, int32_t nphotons,
                    uint32_t detection_state, const uint32_t *d_solid_map,
                    const int32_t *d_solid_id_to_channel_index,
                    const chr_photons *d_out, int32_t *d_out_channels,
                    uint32_t *nhits, void *stream);
/* replaces: count_photons + copy_photons (propagate.cu:70-139) = GPUPhotons.select */
int chr_select_photons(const chr_photons *ph, int32_t start_photon, int32_t nphotons,
                       uint32_t target_flag, const chr_photons *d_out, uint32_t *nselected,
                       void *stream);
/* replaces: copy_photon_queue (propagate.cu:141-169): out[i] = in[queue[i]], i in [first, first+n) */
int chr_copy_photon_queue(const chr_photons *ph, int32_t first_photon, int32_t nphotons,
                          const uint32_t *d_queue, const chr_photons *d_out, void *stream);
/* replaces: photon_duplicate (propagate.cu:29-68): copy photon i to i + stride*c, c=1..copies.
 * evidx must be allocated nphotons*(copies+1) (the reference allocates only n: photon.py:62). */
int chr_photon_duplicate(const chr_photons *ph, int32_t first_photon, int32_t nphotons,
                         int32_t copies, int32_t stride, void *stream);

/* replaces: distance_to_mesh test kernel (chroma/cuda/mesh.h:131-159).
 * d_distance[i] is written only when ray i hits (reference semantics). */
int chr_distance_to_mesh(const chr_geometry *g, uint32_t n, const float *d_origin,
                         const float *d_direction, float *d_distance, void *stream);

/* ------------------------------------------------------------- BVH build */
/* replaces: make_recursive_grid_bvh (chroma/bvh/grid.py:11-95) with its GPU
 * helpers create_leaf_nodes/make_leaves, merge_nodes_detailed/make_parents_detailed,
 * concatenate_layers/copy_and_offset and collapse_chains/collapse_child
 * (chroma/gpu/bvh.py:18-130, chroma/cuda/bvh.cu:148-384,530-543), on the host.
 * Leaves with equal Morton codes keep triangle order (stable sort; the
 * reference's numpy quicksort is unstable).  The result is an opaque handle:
 * query sizes with chr_bvh_result_info, copy out with chr_bvh_result_copy. */
typedef struct chr_bvh_result chr_bvh_result;
int chr_bvh_build_grid(const float *h_vertices, uint32_t nvertices,
                       const uint32_t *h_triangles, uint32_t ntriangles,
                       int32_t target_degree, chr_bvh_result **out);
int chr_bvh_result_info(const chr_bvh_result *r, uint32_t *nnodes, uint32_t *nlayers,
                        float *world_origin /*[3]*/, float *world_scale);
int chr_bvh_result_copy(const chr_bvh_result *r, uint32_t *h_nodes /*[nnodes*4]*/,
                        uint32_t *h_layer_offsets /*[nlayers]*/);
int chr_bvh_result_free(chr_bvh_result *r);

/* ------------------------------------------------------------- flatten helper
 * replaces: the np.unique(rows, return_inverse=True) of Mesh.remove_duplicate_vertices
 * (chroma/geometry.py:71-81, called by Geometry.flatten, geometry.py:337-391)
 * where every set of equal rows is bit-identical (so which duplicate numpy
 * keeps cannot matter): rows sorted lexicographically by float value (x, then
 * y, then z; -0.0 == +0.0), duplicates merged.  out_vertices (>= n rows)
 * receives the unique rows, *nunique their count, inverse[i] the unique row of
 * input row i.  Returns CHR_ERR_INVALID for a NaN, or a set of equal rows that
 * mixes +0.0 and -0.0 (the caller then uses numpy). */
int chr_unique_vertices(const float *h_vertices, uint64_t n, float *h_out_vertices, uint64_t *nunique,
                        int64_t *h_inverse);

/* ------------------------------------------------------------- traversal BVH
 * The layout the gfx950 walk uses (csrc/wide_bvh.h): an 8-wide SAH tree over
 * the reference BVH's own leaf boxes, each triangle carrying its reference DFS
 * rank.  chr_geometry_create builds it internally; these entries expose the
 * same host build for inspection and tests (no reference counterpart: it is
 * a derived acceleration structure, not part of the reference's data).
 * Nodes are 96 bytes, triangle records 64 bytes (see wide_bvh.h). */
typedef struct chr_wide_result chr_wide_result;
int chr_wide_bvh_build(const chr_geometry_desc *desc, chr_wide_result **out);
int chr_wide_bvh_info(const chr_wide_result *r, uint32_t *nnodes, uint32_t *ntri,
                      uint32_t *max_depth, int32_t *usable);
int chr_wide_bvh_copy(const chr_wide_result *r, void *h_nodes /*[nnodes*96 B]*/,
                      void *h_tri /*[ntri*64 B]*/);
int chr_wide_bvh_free(chr_wide_result *r);

/* The traversal BVH in its compact, cacheable form.  The reference caches the
 * BVH its kernel walks, keyed by mesh MD5 (chroma/cache.py:209-236, used by
 * chroma/loader.py:131-160); here the structure the kernel walks is the wide
 * BVH, a function of the mesh and the reference BVH only.  Its compact form
 * keeps what the build decides -- the nodes, each triangle record's triangle
 * id and reference DFS rank -- and drops what the upload
 * derives from the geometry descriptor (vertices, reference leaf words,
 * material codes), so a cached copy cannot go stale against the materials. */
typedef struct chr_wide_bvh_desc {
    uint32_t nnodes;                /* 96-byte nodes (wide_bvh.h WideNode) */
    uint32_t nrec;                  /* triangle records = triangles reachable in the reference BVH */
    uint32_t max_depth;             /* levels below the root */
    int32_t usable;                 /* 0: the wide walk cannot be used (the exact-order walk is) */
    uint32_t leaf_max;              /* builder setting it was built with */
    const void *h_nodes;            /* [nnodes*96 B] */
    const uint32_t *h_rec_id;       /* [nrec] triangle id of record i */
    const uint32_t *h_rec_rank;     /* [nrec] its reference DFS rank (a permutation of [0, nrec)) */
} chr_wide_bvh_desc;
/* sizes and settings of a built result (pointers left NULL) */
int chr_wide_bvh_describe(const chr_wide_result *r, chr_wide_bvh_desc *out);
/* copy the compact form into caller arrays sized by chr_wide_bvh_describe */
int chr_wide_bvh_export(const chr_wide_result *r, void *h_nodes, uint32_t *h_rec_id, uint32_t *h_rec_rank);
/* the builder's settings as a short string ("w<format>-l<leaf max>"):
 * part of a cache key -- a compact form is reused only under the same settings */
int chr_wide_bvh_key(char *out, uint32_t n);
/* check a compact form against a geometry (every index in range, the ranks a
 * permutation, the depth within the walk's stack) and rebuild its 64-byte
 * triangle records [first, first+n) on the host (tests; the upload does the same) */
int chr_wide_bvh_records(const chr_geometry_desc *desc, const chr_wide_bvh_desc *wide, uint32_t first,
                         uint32_t n, void *h_tri /*[n*64 B]*/);
/* chr_geometry_create with a prebuilt (e.g. cached) traversal BVH instead of
 * building it: the same device layout and results, without the build.  The
 * compact form is validated first (CHR_ERR_INVALID if it does not fit desc);
 * one marked unusable selects the exact-order walk, as the build would. */
int chr_geometry_create_wide(const chr_geometry_desc *desc, const chr_wide_bvh_desc *wide,
                             chr_geometry **out);

/* Threads of the library's host-side parallel regions (BVH builds, record
 * fill, vertex merge).  Default: the usable cores (affinity mask capped by the
 * cgroup CPU quota) divided by $LOCAL_WORLD_SIZE; n = 0 restores the default.
 * No reference counterpart (the reference builds on the GPU). */
int chr_set_host_threads(int32_t n);
int32_t chr_get_host_threads(void);

/* ------------------------------------------------------------------- DAQ
 * replaces: chroma/cuda/daq.cu + GPUDaq (chroma/gpu/daq.py:37-101) and the
 * Detector struct (chroma/cuda/detector.h:4-22, uploaded by
 * chroma/gpu/detector.py:21-40).  Per-channel accumulators are u32 arrays of
 * ndaq*nchannels (copy i of channel c at i*stride + c): earliest time as the
 * float's bit pattern under unsigned atomicMin (daq.cu:5-10 keeps
 * float_to_sortable_int as a plain bit cast), charge as round(q/charge_unit)
 * under atomicAdd, history under atomicOr -- all order-independent, so the
 * result does not depend on the schedule. */
typedef struct chr_daq_detector {
    const int32_t *d_solid_id_to_channel_index;   /* [nsolids] */
    const float *d_time_cdf_x, *d_time_cdf_y;     /* [time_cdf_len] */
    const float *d_charge_cdf_x, *d_charge_cdf_y; /* [charge_cdf_len] */
    int32_t nchannels, time_cdf_len, charge_cdf_len;
    float charge_unit;                            /* charge_cdf_x[-1] / 2^16 (gpu/detector.py:39) */
} chr_daq_detector;

/* replaces: GPUDaq.begin_acquire (daq.py:56-60): time words = bits(maxtime), q and history = 0 */
int chr_daq_begin(uint32_t *d_time_int, uint32_t *d_q_int, uint32_t *d_history, uint32_t n, float maxtime,
                  void *stream);
/* replaces: GPUDaq.acquire (daq.py:62-91): run_daq (ndaq == 1, daq.cu:35-83) or
 * run_daq_many (ndaq > 1, daq.cu:85-145) over photons [start, start+n) with the
 * reference's chunking (slot = position in chunk; nthreads_per_block*max_blocks
 * slots for ndaq == 1, one photon per block of nthreads_per_block slots for
 * ndaq > 1).  d_normal_cache (2 words per slot, zero after chr_init_rng) holds
 * curand_normal's cached value; required only for ndaq > 1.  Synchronous. */
int chr_daq_acquire(const chr_photons *ph, uint32_t *d_rng_states, uint32_t rng_nslots, uint32_t *d_normal_cache,
                    uint32_t detection_state, int32_t start_photon, int32_t nphotons,
                    const uint32_t *d_solid_map, const chr_daq_detector *det,
                    uint32_t *d_time_int, uint32_t *d_q_int, uint32_t *d_history,
                    int32_t ndaq, int32_t stride, float global_weight,
                    int32_t nthreads_per_block, int32_t max_blocks, void *stream);
/* replaces: GPUDaq.end_acquire (daq.py:93-101): convert_sortable_int_to_float
 * over all n words, convert_charge_int_to_float over the first nchannels words
 * only (daq.cu:158-172; later DAQ copies keep charge 0, as in the reference). */
int chr_daq_end(const uint32_t *d_time_int, float *d_time, const uint32_t *d_q_int, float *d_q, uint32_t n,
                int32_t nchannels, float charge_unit, void *stream);

/* replaces: the per-event DAQ loop, GPUDaq.begin_acquire / acquire / end_acquire
 * (gpu/daq.py:56-101) as driven once per event by sim.py:143-152.  ndaq = 1 DAQ
 * passes for the nevents consecutive photon ranges [h_bounds[e], h_bounds[e+1])
 * of one chr_photons (h_bounds: nevents+1 non-decreasing host offsets within
 * [0, nphotons]), in a number of launches that does not depend on nevents.
 * Outputs are nevents rows of det->nchannels words, row e = event e: d_time_int
 * (the f32 earliest times' bit patterns, 1e9 where nothing was recorded),
 * d_q_int, d_history, and d_q = d_q_int * charge_unit in EVERY row (each row is
 * its own ndaq = 1 acquisition).  Rows and the RNG slot states afterwards are
 * bit-identical to chr_daq_begin(1e9) + chr_daq_acquire(start = h_bounds[e],
 * n = h_bounds[e+1] - h_bounds[e], ndaq = 1) + chr_daq_end for e = 0, 1, ...:
 * with cap = nthreads_per_block*max_blocks, slot s draws in event e iff
 * s < min(cap, n_e), for positions s, s+cap, ... of it, events ascending.
 * CHR_ERR_INVALID before any launch for null arguments, missing CDFs, nevents
 * < 0, h_bounds decreasing / below 0 / beyond nphotons, min(cap, max n_e) >
 * rng_nslots, or nevents*nchannels > 2^31; nevents == 0 is CHR_OK and touches
 * nothing.  Synchronous. */
int chr_daq_acquire_events(const chr_photons *ph, int32_t nphotons, const int64_t *h_bounds, int32_t nevents,
                           uint32_t *d_rng_states, uint32_t rng_nslots, uint32_t detection_state,
                           const uint32_t *d_solid_map, const chr_daq_detector *det,
                           uint32_t *d_time_int, uint32_t *d_q_int, uint32_t *d_history, float *d_q,
                           float global_weight, int32_t nthreads_per_block, int32_t max_blocks, void *stream);

/* chr_daq_acquire_events for ndaq > 1 (run_daq_many, daq.cu:85-145): the DAQ of
 * ndaq copies for the nevents consecutive photon ranges of h_bounds, in a
 * number of launches that does not depend on nevents.  Outputs are nevents rows
 * of ndaq*nchannels words, row e = event e, copy i of channel c at i*nchannels
 * + c inside it: d_time_int (whose bit view as f32 is what chr_daq_end writes),
 * d_q_int, d_history, and d_q as chr_daq_end after GPUDaq.begin_acquire's fill
 * leaves it (the first nchannels words of a row converted, the rest 0).  Rows,
 * the RNG slot states and d_normal_cache afterwards are bit-identical to
 * chr_daq_begin(1e9) + chr_daq_acquire(start = h_bounds[e], n = h_bounds[e+1] -
 * h_bounds[e], ndaq, stride = nchannels) + chr_daq_end for e = 0, 1, ...: slot
 * tid + nthreads_per_block*b draws in event e iff b < min(max_blocks, n_e), for
 * positions b, b+max_blocks, ... of it and copies tid, tid+nthreads_per_block,
 * ... < ndaq of each detected photon (uniform, normal, time CDF, charge CDF),
 * events ascending.  A channel index at or beyond nchannels counts as not
 * detected (chr_daq_acquire would write it through, into a later copy or row).
 * CHR_ERR_INVALID before any launch for null arguments, missing CDFs, ndaq <
 * 2, nthreads_per_block > 1024, nevents < 0, h_bounds decreasing / below 0 /
 * beyond nphotons, nthreads_per_block*min(max_blocks, max n_e) > rng_nslots, or
 * nevents*ndaq*nchannels > 2^31; nevents == 0 is CHR_OK and touches nothing.
 * Synchronous. */
int chr_daq_acquire_events_many(const chr_photons *ph, int32_t nphotons, const int64_t *h_bounds, int32_t nevents,
                                uint32_t *d_rng_states, uint32_t rng_nslots, uint32_t *d_normal_cache,
                                uint32_t detection_state, const uint32_t *d_solid_map, const chr_daq_detector *det,
                                uint32_t *d_time_int, uint32_t *d_q_int, uint32_t *d_history, float *d_q,
                                int32_t ndaq, float global_weight, int32_t nthreads_per_block, int32_t max_blocks,
                                void *stream);

/* chr_daq_acquire_events that also keeps what it draws: one photoelectron
 * record per photon of the span [h_bounds[0], h_bounds[nevents]), indexed from
 * the span's first photon (record i belongs to photon h_bounds[0] + i), in three
 * device arrays of that many entries.  Every record is written: a photon the DAQ
 * accepts (selected as a candidate, its uniform below weight * global_weight)
 * gets its channel in d_pe_channel, the float time handed to the earliest-time
 * minimum in d_pe_time and its quantised charge word in d_pe_q; every other
 * photon gets -1, the 1e9 no-hit time and 0.  A photon makes at most one
 * photoelectron, so the records need no atomics and come in photon order.  The
 * channel rows, d_q and the RNG slot states afterwards are bit-identical to
 * chr_daq_acquire_events on the same inputs: the same slots, chunks and events
 * walked, the same draws in the same order -- the same stream.  Folding the
 * records per (event, channel) gives the rows back: unsigned minimum of the
 * times' bit patterns, sum of the charge words mod 2^32 (the history is the OR
 * of the accepted photons' flags).  The candidate pass always runs
 * (CHR_DAQ_EVENTS_SHAPE applies to chr_daq_acquire_events only).  Refusals as
 * chr_daq_acquire_events, and a null record array; all before any launch.
 * Synchronous. */
int chr_daq_acquire_events_pe(const chr_photons *ph, int32_t nphotons, const int64_t *h_bounds, int32_t nevents,
                              uint32_t *d_rng_states, uint32_t rng_nslots, uint32_t detection_state,
                              const uint32_t *d_solid_map, const chr_daq_detector *det,
                              uint32_t *d_time_int, uint32_t *d_q_int, uint32_t *d_history, float *d_q,
                              int32_t *d_pe_channel, float *d_pe_time, uint32_t *d_pe_q,
                              float global_weight, int32_t nthreads_per_block, int32_t max_blocks, void *stream);

/* Detected photons per channel, ACCUMULATED into d_counts[nchannels] (u32; the
 * caller zeroes it): the selection of count_photon_hits (propagate.cu:172-199)
 * histogrammed by channel.  No reference counterpart -- it is the per-rank
 * array a photon-sharded run reduces over RCCL (chroma/gpu/shard.py). Async. */
int chr_channel_hit_counts(const chr_photons *ph, int32_t start_photon, int32_t nphotons,
                           uint32_t detection_state, const uint32_t *d_solid_map,
                           const int32_t *d_solid_id_to_channel_index, uint32_t *d_counts,
                           int32_t nchannels, void *stream);

/* ---------------------------------------------------------------- hit maps
 * A hit map is the table "source s flashed N photons: how many reached channel
 * c, when did the first arrive, how are the arrival times distributed" -- the
 * optical map (photon library) of fast simulation and reconstruction.  The
 * source of a photon is its evidx (a genstep's evidx is the caller's absolute
 * source id; chr_generate_photons stamps it and the propagator leaves it
 * alone).  No reference counterpart: the reference builds such a table on the
 * host from one event per source.
 *
 * Arrays (device for chr_hitmap_clear / chr_hitmap_accumulate, host for
 * chr_hitmap_accumulate_host), each of at most 2^31 words:
 *   d_emitted[nsources]                    u64, required
 *   d_counts[nsources*nchannels]           u32, required
 *   d_tmin[nsources*nchannels]             u32, optional (NULL: not kept)
 *   d_thist[nsources*nchannels*ntbins]     u32, present exactly when ntbins > 0
 *   d_wsum[nsources*nchannels]             u64, optional (NULL: not kept)
 *   d_skipped                              one u64 word, required
 * t_lo and inv describe the time histogram: inv = ntbins / (t_hi - t_lo),
 * computed once by the caller in float32.
 *
 * The rule, for photon p, in this order (csrc/hitmap.h, one text for the
 * device and the host twin):
 *   1. s = evidx[p]; s >= nsources: skipped += 1, stop.
 *   2. emitted[s] += 1, detected or not (the denominator of the visibility).
 *   3. the channel, as chr_channel_hit_counts selects it: flags[p] &
 *      detection_state, last_hit[p] > -1, c = s2c[solid_map[last_hit[p]]] with
 *      0 <= c < nchannels; otherwise stop.
 *   4. w = s*nchannels + c; counts[w] += 1.
 *   5. d_tmin kept and t[p] not NaN: tmin[w] = min(tmin[w], key), unsigned,
 *      key = the order-preserving form of the float's bits b: b ^ 0xFFFFFFFF
 *      when the sign bit is set, else b ^ 0x80000000 (negative times sort below
 *      positive ones, unlike the DAQ's raw-bits min).  Cleared word: 0xFFFFFFFF.
 *   6. ntbins > 0: x = (t[p] - t_lo) * inv, one float32 subtract and one
 *      float32 multiply, never contracted; x >= 0.0f && x < (float)ntbins:
 *      thist[w*ntbins + (uint32_t)x] += 1.  NaN and infinite times fail the
 *      test; there are no under- or overflow bins.
 *   7. d_wsum kept: wsum[w] += q, q = (uint64_t)(weight[p] * 16777216.0f)
 *      truncated; 0 for a NaN or negative weight, 2^32 - 1 when the product is
 *      >= 4294967296.0f.
 * Every update is an integer add or an unsigned min, so a map is a function of
 * its photons alone, bit for bit, whatever their order, the path taken or the
 * split into calls; maps add over calls (SUM; MIN for tmin). */
typedef struct chr_hitmap_desc {
    uint32_t nsources;
    int32_t nchannels;
    uint32_t ntbins;              /* 0: no time histogram */
    float t_lo, inv;
    uint64_t *d_emitted;
    uint32_t *d_counts, *d_tmin, *d_thist;
    uint64_t *d_wsum, *d_skipped;
} chr_hitmap_desc;
/* words of one source's row the privatised path of chr_hitmap_accumulate keeps in LDS (32 KB) */
#define CHR_HITMAP_LDS_WORDS 8192

/* Zero every array of the map and set d_tmin to 0xFFFFFFFF.  CHR_ERR_INVALID before
 * the launch for what chr_hitmap_accumulate refuses of a map.  Async. */
int chr_hitmap_clear(const chr_hitmap_desc *desc, void *stream);
/* Add photons [start_photon, start_photon + nphotons) of ph to the map by the rule
 * above; ph is only read (evidx, flags, last hits; t when d_tmin or d_thist is kept,
 * weights when d_wsum is).  d_solid_map / d_solid_id_to_channel_index as in
 * chr_channel_hit_counts.  Two paths with identical words: rule steps 4-7 straight
 * into global memory, or, when one source's row (nchannels * (1 + [tmin] + ntbins +
 * 2*[wsum]) words) fits CHR_HITMAP_LDS_WORDS, into an LDS copy of the row of the
 * workgroup's current source that is swept out when the source changes (the default
 * then for a map with a time histogram or weight sums, the direct path for counts and
 * tmin alone; the environment's CHR_HITMAP_PATH=d|l forces one, and l with a row over
 * the budget falls back to d).  Correctness does not depend on the photons being sorted
 * by source; the speed does.  CHR_ERR_INVALID before the first launch for: a null
 * required pointer (ph, its evidx / flags / last hits, its t or weights where read,
 * the two maps, desc, d_emitted, d_counts, d_skipped); d_thist null while ntbins > 0
 * or non-null while ntbins == 0; nsources == 0 or nchannels <= 0; an array over 2^31
 * words; inv not finite or not positive while ntbins > 0; start_photon < 0.
 * nphotons <= 0 is CHR_OK and touches nothing.  Async on `stream`. */
int chr_hitmap_accumulate(const chr_photons *ph, int32_t start_photon, int32_t nphotons, uint32_t detection_state,
                          const uint32_t *d_solid_map, const int32_t *d_solid_id_to_channel_index,
                          const chr_hitmap_desc *desc, void *stream);
/* The path of the calling thread's last chr_hitmap_accumulate that launched:
 * 0 direct, 1 privatised, -1 none yet. */
int chr_hitmap_last_path(void);
/* The same on the host (no GPU needed): every pointer of ph, the two maps and desc
 * addresses HOST memory.  Word-identical to chr_hitmap_accumulate (one source,
 * csrc/hitmap.h), with the same refusals. */
int chr_hitmap_accumulate_host(const chr_photons *ph, int32_t start_photon, int32_t nphotons,
                               uint32_t detection_state, const uint32_t *h_solid_map,
                               const int32_t *h_solid_id_to_channel_index, const chr_hitmap_desc *desc);

/* ---------------------------------------------------------------- waveforms
 * The pulse train behind a channel's one time and one charge: the photoelectron
 * records of chr_daq_acquire_events_pe binned into charge trains per (event,
 * channel) row, and the trains convolved with a single-photoelectron template
 * and quantised to ADC words.  No reference counterpart: the reference's DAQ
 * keeps the earliest time and the summed charge only.  Nothing here draws a
 * random number (electronic noise would need draws and a stream contract of its
 * own: it is not modelled).
 *
 * Trains.  The window is (t_lo, inv, nsamples) with inv = nsamples / (t_hi -
 * t_lo) computed once by the caller in float32, as a hit map's.  Arrays (device
 * for chr_daq_pe_trains, host for chr_daq_pe_trains_host):
 *   pe_channel, pe_time, pe_q   the records, h_bounds[nevents] - h_bounds[0] each
 *   row_of_word[nevents*nchannels]  i32, optional (NULL: every word has its row)
 *   trains[nrows*nsamples]      u32, at most 2^31 words
 *   outside_q[nrows]            u32
 *   dropped                     one u32 word
 * The call first zeroes trains, outside_q and dropped.  Then, for record i of
 * the span, in this order (csrc/waveform.h, one text for the device and the
 * host twin):
 *   1. c = pe_channel[i]; c < 0: no photoelectron, stop.  c >= nchannels:
 *      dropped += 1, stop.
 *   2. e = the event of photon h_bounds[0] + i: h_bounds[e] <= it < h_bounds[e+1].
 *   3. w = e*nchannels + c; row = row_of_word[w], or w without a map (nrows must
 *      then be nevents*nchannels).  row < 0 or row >= nrows: dropped += 1, stop.
 *   4. the time bin of the hit map's rule step 6 (csrc/hitmap.h, the same
 *      function): x = (pe_time[i] - t_lo) * inv, one float32 subtract and one
 *      float32 multiply, never contracted; x >= 0.0f && x < (float)nsamples:
 *      trains[row*nsamples + (uint32_t)x] += pe_q[i].  A time exactly t_lo is
 *      in bin 0.
 *   5. otherwise (before the window, at or after its upper edge, infinite or
 *      NaN): outside_q[row] += pe_q[i].
 * Every update is an integer add mod 2^32, so the words are a function of the
 * records alone, whatever the order, and for every row that the map gives
 * exactly the records of one (event, channel)
 *   sum_b trains[row][b] + outside_q[row] == q_int[event][channel]  (mod 2^32)
 * with q_int the charge word chr_daq_acquire_events_pe left for it.
 * CHR_ERR_INVALID before anything is read or launched for: a null required
 * pointer; nevents < 0 or nchannels <= 0; nsamples == 0; t_lo or inv not
 * finite, inv <= 0; nevents*nchannels or nrows*nsamples above 2^31; bounds
 * negative, decreasing or beyond 2^31; no map and nrows != nevents*nchannels.
 * Synchronous. */
int chr_daq_pe_trains(const int32_t *d_pe_channel, const float *d_pe_time, const uint32_t *d_pe_q,
                      const int64_t *h_bounds, int32_t nevents, int32_t nchannels, const int32_t *d_row_of_word,
                      uint32_t nrows, float t_lo, float inv, uint32_t nsamples, uint32_t *d_trains,
                      uint32_t *d_outside_q, uint32_t *d_dropped, void *stream);
/* The same on the host (no GPU needed): every pointer addresses HOST memory.
 * Word-identical to chr_daq_pe_trains, with the same refusals. */
int chr_daq_pe_trains_host(const int32_t *h_pe_channel, const float *h_pe_time, const uint32_t *h_pe_q,
                           const int64_t *h_bounds, int32_t nevents, int32_t nchannels, const int32_t *h_row_of_word,
                           uint32_t nrows, float t_lo, float inv, uint32_t nsamples, uint32_t *h_trains,
                           uint32_t *h_outside_q, uint32_t *h_dropped);

/* words of LDS one row may take in chr_daq_digitise: nsamples + min(ntaps, nsamples) (64 KB) */
#define CHR_WAVE_LDS_WORDS 16384

/* Digitiser.  adc[nrows*nsamples] (u16) from trains[nrows*nsamples], a
 * single-photoelectron template of ntaps floats, scale (the caller's charge
 * unit times gain, folded into one float), pedestal and adc_max <= 65535.  The
 * call first zeroes the one-word `bad`.  Then, for sample s of a row
 * (csrc/waveform.h, one text for both sides):
 *   1. a row whose train is all zero: v = 0 for every sample, without step 2-3.
 *   2. v = 0; for k = 0 .. min(ntaps - 1, s), ascending:
 *   3.     v = fmaf(template[k], (float)trains[row][s - k], v), single-rounded.
 *   4. x = fmaf(v, scale, pedestal); x NaN: adc = 0 and bad += 1.
 *   5. otherwise adc = min(sat_u32(x + 0.5f), adc_max), sat_u32 the saturating
 *      conversion of the DAQ's charge words (negatives give 0).
 * Rows are independent.  CHR_ERR_INVALID before anything is read or launched
 * for: a null pointer; nsamples == 0 or ntaps == 0; nrows*nsamples above 2^31;
 * nsamples + min(ntaps, nsamples) above CHR_WAVE_LDS_WORDS; adc_max > 65535.
 * Async on `stream`. */
int chr_daq_digitise(const uint32_t *d_trains, uint32_t nrows, uint32_t nsamples, const float *d_template,
                     uint32_t ntaps, float scale, float pedestal, uint32_t adc_max, uint16_t *d_adc, uint32_t *d_bad,
                     void *stream);
/* The same on the host (no GPU needed), word-identical, with the same refusals. */
int chr_daq_digitise_host(const uint32_t *h_trains, uint32_t nrows, uint32_t nsamples, const float *h_template,
                          uint32_t ntaps, float scale, float pedestal, uint32_t adc_max, uint16_t *h_adc,
                          uint32_t *h_bad);

/* --------------------------------------------------------- photon library
 * The consumer of a hit map: from the map of a set of sources (the library,
 * a chr_hitmap_desc used READ-ONLY: emitted, counts, optional tmin, optional
 * thist with t_lo and inv; wsum and d_skipped are ignored) and the entries of
 * some events, every event's per-channel expected charge and earliest time
 * (chr_library_expect), or a sampled charge and time per channel
 * (chr_library_sample), without propagating a photon.  No reference
 * counterpart.
 *
 * The entries are a CSR table: event e owns entries offsets[e] ..
 * offsets[e+1]-1 (offsets ascending), entry i says "nphotons[i] photons were
 * made at time t[i] where source source[i] was flashed".  An event's entries
 * are used in the order given.
 *
 * Expected values, for event e and channel c (csrc/library.h, one text for
 * the device, the host twin and, restated, tests/library_model.py):
 *   1. mu = 0.0f, tfirst = +inf.
 *   2. for the entries i of e in order, s = source[i]:
 *   3.   s >= nsources: the entry adds nothing and is counted once (per entry,
 *        not per channel) in *skipped; emitted[s] == 0: it adds nothing.
 *   4.   w = (float)nphotons[i] / (float)emitted[s], one IEEE divide of two
 *        round-to-nearest conversions; k = counts[s*nchannels + c];
 *        mu = fmaf(w, (float)k, mu).
 *   5.   tmin kept, k > 0 and key = tmin[s*nchannels + c] != 0xFFFFFFFF:
 *        cand = t[i] + time_of_key(key) (the hit map's key undone: key ^
 *        0x80000000 when its top bit is set, else key ^ 0xFFFFFFFF, as float
 *        bits); tfirst = cand when cand < tfirst, so a NaN is never taken.
 * mu[e*nchannels + c] and, only when the library keeps tmin,
 * tfirst[e*nchannels + c] are written; every word has one writer, there is no
 * RNG and no atomic but *skipped, so the outputs are a function of the inputs
 * alone, bit for bit.
 *
 * Sampled channels.  Pairs are numbered k = e*nchannels + c, npairs =
 * nevents*nchannels.  T = min(nslots, npairs) work-items run; work-item j loads
 * rng slot j once, handles pairs j, j+T, j+2T, ... in ascending order and
 * stores the state back; slots >= T are untouched.  For a pair: n = 0, mu and
 * tfirst as above, tdrawn = +inf, an empty chr_normal cache (local to the pair,
 * dropped after it); then for the entries in order, those of step 3 skipped:
 *   1. m = w * (float)k, one multiply.
 *   2. n_i = poisson(m): m NaN or <= 0: 0, nothing drawn.  m < 32: Knuth's
 *      product, p = 1, count factors p *= chr_uniform01() until p <=
 *      chr_expf(-m) (at most 1024 factors), n_i = factors - 1.  Otherwise
 *      n_i = chr_sat_u32(fmaf(sqrtf(m), z, m) + 0.5f), z = chr_normal(): a
 *      normal approximation rounded to the nearest integer, negatives to 0,
 *      2^32 and above to 2^32-1.  n = min(n + n_i, 2^32-1).
 *   3. thist kept and n_i > 0: total = the sum of the ntbins words of (s, c)
 *      (uint32); total > 0: for each of the first min(n_i,
 *      CHR_LIBRARY_MAX_TIME_DRAWS) photons: u = chr_uniform01(), r =
 *      min(chr_sat_u32(u * (float)total), total-1), b = the first bin whose
 *      running integer sum exceeds r, x = (float)b + chr_uniform01(), cand =
 *      t[i] + fmaf(x, width, t_lo) with width = 1.0f / inv; tdrawn = cand when
 *      cand < tdrawn.  The cap is an approximation: an entry that gives a
 *      channel more than 64 photons takes the earliest of 64 drawn times, not
 *      of n_i, so the earliest time of a bright channel is biased late by at
 *      most the spread of the 64-sample minimum.
 * n_out[k] = n; t_out[k] = 1e9f (the DAQ's time of a channel without a hit)
 * when n == 0, else tdrawn when thist is kept, else tfirst (+inf when the
 * library holds no time for the pair). */
typedef struct chr_library_entries {
    uint32_t nevents;
    const uint32_t *offsets;          /* nevents + 1 */
    const uint32_t *source, *nphotons;/* per entry */
    const float *t;                   /* per entry */
} chr_library_entries;
#define CHR_LIBRARY_MAX_TIME_DRAWS 64u

/* Expected values by the rule above; *d_skipped (u64) is ADDED to.  d_tfirst
 * may be NULL when the library keeps no tmin.  Two paths with identical words:
 * wide (4 channels per lane through 16-byte loads; nchannels a multiple of 4
 * and counts, tmin, mu, tfirst 16-byte aligned) and narrow (1 channel per
 * lane); the environment's CHR_LIBRARY_PATH=n forces the narrow one.
 * CHR_ERR_INVALID before anything is read through a pointer for: a null
 * required pointer (desc, entries, d_emitted, d_counts, d_mu, d_skipped,
 * d_tfirst while tmin is kept; offsets, source, nphotons, t while nevents >
 * 0); d_thist null while ntbins > 0 or non-null while ntbins == 0; nsources ==
 * 0 or nchannels <= 0; an array over 2^31 words (the map's, or nevents *
 * nchannels); inv not finite or not positive while ntbins > 0.  The device
 * entries do not read offsets on the host: the caller passes them ascending
 * (chroma.library.LibraryEntries checks; the host twins check and refuse).
 * nevents == 0 is CHR_OK and touches nothing.  Async on `stream`. */
int chr_library_expect(const chr_hitmap_desc *lib, const chr_library_entries *entries, float *d_mu, float *d_tfirst,
                       uint64_t *d_skipped, void *stream);
/* The path of the calling thread's last chr_library_expect that launched:
 * 0 narrow, 1 wide, -1 none yet. */
int chr_library_last_path(void);
/* Sampled channels by the rule above: d_n[npairs] u32, d_t[npairs] f32,
 * d_rng_states as chr_init_rng makes them (6 * nslots words), *d_skipped added
 * to.  The refusals of chr_library_expect, d_n / d_t / d_rng_states required,
 * and nslots == 0 or 6 * nslots > 2^31.  Async on `stream`. */
int chr_library_sample(const chr_hitmap_desc *lib, const chr_library_entries *entries, uint32_t *d_rng_states,
                       uint32_t nslots, uint32_t *d_n, float *d_t, uint64_t *d_skipped, void *stream);
/* The same on the host (no GPU needed): every pointer addresses HOST memory.
 * Word-identical to the device entries (one source, csrc/library.h), with the
 * same refusals and one more: offsets not ascending. */
int chr_library_expect_host(const chr_hitmap_desc *lib, const chr_library_entries *entries, float *h_mu,
                            float *h_tfirst, uint64_t *h_skipped);
int chr_library_sample_host(const chr_hitmap_desc *lib, const chr_library_entries *entries, uint32_t *h_rng_states,
                            uint32_t nslots, uint32_t *h_n, float *h_t, uint64_t *h_skipped);

/* Log-likelihood: the way back.  One observed event (nobs, optional tobs) is
 * scored against many hypotheses straight from the library; hypothesis h is
 * "event" h of a chr_library_entries table, and eight bytes per hypothesis are
 * written.  The rule (csrc/library.h, one text for the device, the host twin
 * and, restated, tests/loglike_model.py), LIMIT = 8388608.0f (2^23), for
 * hypothesis h and channel c, in this order:
 *   1. mu exactly as steps 1-4 of the expected values: the same w, the same
 *      fmaf fold in entry order, so mu is the word chr_library_expect stores.
 *      With tobs given and nobs[c] > 0, also a = 0.0f folded over the same
 *      counted entries: b = the hit map's time bin (rule step 6 there) of
 *      tobs[c] - t[i], one float32 subtract; b >= 0:
 *      a = fmaf(w, (float)thist[(s*nchannels + c)*ntbins + b], a).
 *   2. m = mu + floor, one float32 add; n = nobs[c].
 *   3. the charge term:
 *        !(m > 0) (zero, negative, NaN):  term = n == 0 ? 0.0f : -LIMIT
 *        n == 0:                          term = -m
 *        mode 0 (Poisson):                term = fmaf((float)n, chr_logf(m), -m)
 *        mode 1 (hit / no hit):           p = 1.0f - chr_expf(-m);
 *                                         term = p > 0 ? chr_logf(p) : -LIMIT
 *      The Poisson form's lgamma(n + 1) is the same for every hypothesis and
 *      is LEFT OUT: ll is the log-likelihood up to that constant.
 *   4. the time term, only with tobs given, n > 0, m > 0 and tobs[c] not NaN:
 *      d = fmaf(a, inv, tfloor);
 *      term = (term + (d > 0 ? chr_logf(d) : -LIMIT)) - chr_logf(m), two
 *      float32 operations in that order: the single-photon arrival density of
 *      the mixture "library signal plus flat noise", normalised when tfloor =
 *      floor / (t_hi - t_lo).
 *   5. the word: a NaN term gives q = 0 and adds 1 to bad[h]; otherwise the
 *      term is clamped to [-LIMIT, LIMIT] and q = (int64_t)(term *
 *      1048576.0f), truncated toward zero (the product is exact).
 *   6. ll[h] += q, a 64-bit INTEGER add.
 * A sum of integers does not depend on how the channels are spread over
 * lanes, waves and workgroups, so ll and bad are functions of the inputs
 * alone, bit for bit (as a hit map is).  |q| <= 2^43 and nchannels <= 2^20, so
 * the sum cannot overflow; ll[h] / 2^20 is the log-likelihood, resolved to
 * 1e-6 per channel.  An entry of a source >= nsources adds nothing and is
 * counted once in *skipped, as in chr_library_expect. */
typedef struct chr_library_observed {
    const uint32_t *nobs;   /* nchannels: photo-electron counts, or 0 / 1 for hit / no hit */
    const float *tobs;      /* nchannels: the time of a hit channel; or NULL: no time term */
    uint32_t mode;          /* 0 Poisson, 1 hit / no hit */
    float floor, tfloor;    /* expected noise charge per channel; noise time density (read with tobs) */
} chr_library_observed;
/* d_ll[nevents] (int64) and d_bad[nevents] (u32) are WRITTEN: they are zeroed on
 * `stream` before the kernel; *d_skipped (u64) is ADDED to.  Two paths with
 * identical words: wide (4 channels per lane; tobs NULL, nchannels a multiple
 * of 4 and counts, nobs 16-byte aligned) and narrow (always with tobs, where
 * the histogram gather decides the time); the environment's
 * CHR_LIBRARY_PATH=n forces the narrow one.  CHR_ERR_INVALID before anything is
 * read through a pointer for everything chr_library_expect refuses of the
 * library and the table (nevents * nchannels > 2^31 among it: inherited, so
 * that one check serves every entry; this call writes 12 bytes per hypothesis
 * and has no table of that size -- split larger tables), and for: a null obs, nobs, d_ll or d_bad; mode > 1;
 * floor or tfloor NaN or negative; tobs non-null while the library keeps no
 * thist; nchannels > 2^20.  nevents == 0 is CHR_OK and touches nothing.  Async
 * on `stream`. */
int chr_library_loglike(const chr_hitmap_desc *lib, const chr_library_entries *hyp, const chr_library_observed *obs,
                        int64_t *d_ll, uint32_t *d_bad, uint64_t *d_skipped, void *stream);
/* The path of the calling thread's last chr_library_loglike that launched:
 * 0 narrow, 1 wide, -1 none yet. */
int chr_library_loglike_last_path(void);
/* The same on the host (every pointer addresses HOST memory), word-identical,
 * with the same refusals and one more: offsets not ascending. */
int chr_library_loglike_host(const chr_hitmap_desc *lib, const chr_library_entries *hyp,
                             const chr_library_observed *obs, int64_t *h_ll, uint32_t *h_bad, uint64_t *h_skipped);

/* ------------------------------------------------------------------- PDF
 * replaces: chroma/cuda/pdf.cu, launched by GPUPDF / GPUKernelPDF
 * (chroma/gpu/pdf.py:7-372).  Inputs are GPUChannels words (t, q: f32; DAQ
 * copy i of channel c at i*nchannels + c).  One work-item per channel, the
 * reference's accumulation order and float accumulators.  All async. */

/* replaces: bin_hits (pdf.cu:9-32; GPUPDF.add_hits_to_pdf, pdf.py:206-222).
 * d_pdf is [nchannels][tbins][qbins] u32.  Bins are clamped to the channel's
 * last bin (the reference can spill t == tmax-ulp into the next row). */
int chr_pdf_bin_hits(int32_t nchannels, const float *d_channel_q, const float *d_channel_time,
                     uint32_t *d_hitcount, int32_t tbins, float tmin, float tmax, int32_t qbins, float qmin,
                     float qmax, uint32_t *d_pdf, void *stream);
/* chr_pdf_bin_hits for nrows consecutive rows of nchannels words (row r of
 * channel c at r*nchannels + c in d_channel_q / d_channel_time): one work-item
 * per channel walks the rows in order; d_hitcount and d_pdf afterwards equal
 * nrows calls of chr_pdf_bin_hits, one per row.  No reference counterpart. */
int chr_pdf_bin_hits_rows(int32_t nchannels, int32_t nrows, const float *d_channel_q, const float *d_channel_time,
                          uint32_t *d_hitcount, int32_t tbins, float tmin, float tmax, int32_t qbins, float qmin,
                          float qmax, uint32_t *d_pdf, void *stream);
/* replaces: accumulate_bincount (pdf.cu:34-96; GPUPDF.accumulate_pdf_eval,
 * pdf.py:296-316).  d_work_queues: nhit*(ndaq+1) u32, word 0 of each queue
 * = 1 + queued entries (the caller fills 1). */
int chr_pdf_accumulate_bincount(int32_t nchannels, int32_t ndaq, const uint32_t *d_event_hit,
                                const float *d_event_time, const float *d_mc_time, uint32_t *d_hitcount,
                                uint32_t *d_bincount, float min_twidth, float tmin, float tmax,
                                int32_t min_bin_content, const uint32_t *d_map_channel_to_hit,
                                uint32_t *d_work_queues, void *stream);
/* replaces: accumulate_nearest_neighbor_block (pdf.cu:152-219; pdf.py:318-328):
 * per hit, the min_bin_content smallest of (stored table + queued distances),
 * ascending.  min_bin_content <= 8192 (the reference's table holds 1000). */
int chr_pdf_accumulate_nearest(int32_t nhit, int32_t ndaq, const uint32_t *d_map_hit_to_channel,
                               const uint32_t *d_work_queues, const float *d_event_time,
                               const float *d_mc_time, float *d_nearest_mc, int32_t min_bin_content,
                               void *stream);
/* replaces: accumulate_moments (pdf.cu:223-266; GPUKernelPDF.accumulate_moments, pdf.py:42-59) */
int chr_pdf_accumulate_moments(int32_t time_only, int32_t nchannels, const float *d_mc_time,
                               const float *d_mc_charge, float tmin, float tmax, float qmin, float qmax,
                               uint32_t *d_mom0, float *d_t_mom1, float *d_t_mom2, float *d_q_mom1,
                               float *d_q_mom2, void *stream);
/* replaces: accumulate_kernel_eval (pdf.cu:271-368; GPUKernelPDF.accumulate_kernel, pdf.py:139-158) */
int chr_pdf_accumulate_kernel_eval(int32_t time_only, int32_t nchannels, const uint32_t *d_event_hit,
                                   const float *d_event_time, const float *d_event_charge,
                                   const float *d_mc_time, const float *d_mc_charge, float tmin, float tmax,
                                   float qmin, float qmax, const float *d_inv_time_bw,
                                   const float *d_inv_charge_bw, uint32_t *d_hitcount, float *d_time_pdf,
                                   float *d_charge_pdf, void *stream);

/* ---------------------------------------------------------------- renderer
 * replaces: the `render` kernel (chroma/cuda/render.cu:37-183) as launched by
 * GPURays.render (chroma/gpu/render.py:47-62).  Rays float3-packed [n*3] (not
 * normalised, as the reference); d_colors: one ARGB word per triangle
 * (reference GPUGeometry.colors); per ray: d_dx / d_color (float4) hold
 * alpha_depth entries, d_dxlen the entries kept (0 = start afresh; a
 * non-zero count merges this render into the previous one, keep_last_render).
 * d_pixels[i] = composited ARGB or bg_color. */
int chr_render(const chr_geometry *g, uint32_t nrays, const float *d_pos, const float *d_dir,
               const uint32_t *d_colors, uint32_t alpha_depth, uint32_t *d_pixels, float *d_dx,
               uint32_t *d_dxlen, float *d_color, uint32_t bg_color, void *stream);
/* replaces: transform.cu:9-48 (translate / rotate / rotate_around_point of float3 arrays,
 * GPURays.translate/rotate/rotate_around_point, gpu/render.py:30-45) */
int chr_transform_translate(uint32_t n, float *d_a, float vx, float vy, float vz, void *stream);
int chr_transform_rotate(uint32_t n, float *d_a, float phi, float ax, float ay, float az, void *stream);
int chr_transform_rotate_around_point(uint32_t n, float *d_a, float phi, float ax, float ay, float az,
                                      float px, float py, float pz, void *stream);
/* replaces: hybrid_render.cu:61-131 update_xyz_lookup (camera.py:246-258): work-item k
 * (k < nthreads, triangle id = k + offset < total_threads, RNG slot k) shoots light from
 * position[3] at a random point of its triangle; if that triangle is the first hit, the
 * photon is propagated to its first diffuse reflection and cos_theta * xyz[3] is added to
 * the reflecting triangle's float3 entry of d_lookup1 (inside-to-outside) or d_lookup2.
 * d_vertices / d_triangles: the mesh (float3 / uint3 packed). */
int chr_hybrid_update_xyz_lookup(const chr_geometry *g, const float *d_vertices, const uint32_t *d_triangles,
                                 int32_t nthreads, int32_t total_threads, int32_t offset, const float *position,
                                 uint32_t *d_rng_states, uint32_t rng_nslots, float wavelength, const float *xyz,
                                 float *d_lookup1, float *d_lookup2, int32_t max_steps, void *stream);
/* replaces: hybrid_render.cu:133-166 update_xyz_image (camera.py:260-275) */
int chr_hybrid_update_xyz_image(const chr_geometry *g, int32_t nthreads, uint32_t *d_rng_states,
                                uint32_t rng_nslots, const float *d_positions, const float *d_directions,
                                float wavelength, const float *xyz, const float *d_lookup1,
                                const float *d_lookup2, float *d_image, int32_t nlookup_calls,
                                int32_t max_steps, void *stream);
/* replaces: hybrid_render.cu:168-200 process_image (camera.py:277-282) */
int chr_hybrid_process_image(int32_t nthreads, const float *d_image, uint32_t *d_pixels, int32_t nimages,
                             void *stream);

/* ------------------------------------------------------------ self tests
 * The reference's unit-test kernels, run over this build's device math (the
 * functions the propagate kernels inline).  Tests only. */
enum chr_linalg_op {   /* replaces: the 20 kernels of test/linalg_test.cu, in order */
    CHR_LINALG_FLOAT3ADD = 0, CHR_LINALG_FLOAT3ADDEQUAL, CHR_LINALG_FLOAT3SUB, CHR_LINALG_FLOAT3SUBEQUAL,
    CHR_LINALG_FLOAT3ADDFLOAT, CHR_LINALG_FLOAT3ADDFLOATEQUAL, CHR_LINALG_FLOATADDFLOAT3, CHR_LINALG_FLOAT3SUBFLOAT,
    CHR_LINALG_FLOAT3SUBFLOATEQUAL, CHR_LINALG_FLOATSUBFLOAT3, CHR_LINALG_FLOAT3MULFLOAT,
    CHR_LINALG_FLOAT3MULFLOATEQUAL, CHR_LINALG_FLOATMULFLOAT3, CHR_LINALG_FLOAT3DIVFLOAT,
    CHR_LINALG_FLOAT3DIVFLOATEQUAL, CHR_LINALG_FLOATDIVFLOAT3, CHR_LINALG_DOT, CHR_LINALG_CROSS, CHR_LINALG_NORM,
    CHR_LINALG_MINUSFLOAT3, CHR_LINALG_NOPS
};
/* d_a, d_b: float3-packed [n*3]; d_out [n*3] (or [n] for DOT/NORM) */
int chr_selftest_linalg(int32_t op, uint32_t n, const float *d_a, const float *d_b, float c, float *d_out,
                        void *stream);
/* replaces: test/rotate_test.cu (rotate.h:21-28): d_out[i] = rotate(a[i], phi[i], n) */
int chr_selftest_rotate(uint32_t n, const float *d_a, const float *d_phi, float nx, float ny, float nz,
                        float *d_out, void *stream);
/* The functions of chroma_fmath.h and the IEEE primitives they rest on (sqrt, fma, plain
 * division, each compiled with the library's own flags), one op per launch: the device side of
 * the header's claim that gfx950 and the host oracle compute the same bits
 * (tests/test_gpu_fmath.py; the oracle's orc_math_bits is the host side, same numbering). */
enum chr_fmath_op {
    CHR_FMATH_LOG = 0, CHR_FMATH_EXP, CHR_FMATH_SIN, CHR_FMATH_COS, CHR_FMATH_TAN, CHR_FMATH_ASIN, CHR_FMATH_ACOS,
    CHR_FMATH_ATAN2,        /* chr_atan2f(y, x) */
    CHR_FMATH_ATAN, CHR_FMATH_ERF,
    CHR_FMATH_LDEXP,        /* chr_ldexpf(x, k), y carrying the integer k as a float (CHR_FMATH_LDEXP_K) */
    CHR_FMATH_SAT_U32,      /* the result word is the integer itself */
    CHR_FMATH_RINT_SMALL, CHR_FMATH_SQRT,
    CHR_FMATH_FMA,          /* fma(x, y, x) */
    CHR_FMATH_DIV,          /* x / y */
    CHR_FMATH_NOPS
};
/* For this self test and its host twin (orc_math_bits) only, not for callers of the library: ldexp's
 * exponent from its float carrier, a defined conversion for every y (0 outside +-4096 and for NaN) */
#define CHR_FMATH_LDEXP_K(y) (((y) >= -4096.0f && (y) <= 4096.0f) ? (int)(y) : 0)
/* d_out_bits[i] = the bit pattern of op(d_x[i], d_y[i]), i < n; one-argument ops read d_y too
 * (any values).  Unknown op or null pointer: CHR_ERR_INVALID; n == 0 succeeds. */
int chr_selftest_fmath(int32_t op, uint32_t n, const float *d_x, const float *d_y, uint32_t *d_out_bits,
                       void *stream);
/* replaces: test/test_sample_cdf.cu (random.h:27-55): one draw per slot i < n from
 * RNG slot state i (SoA, chr_init_rng layout; states are not written back);
 * uniform_grid = 0: sample_cdf(cdf_x, cdf_y), 1: sample_cdf(x0, delta, cdf_y),
 * 2: the bucket-indexed form of 1 the propagate kernels use for re-emission time
 * CDFs (index built as chr_geometry_create builds it; synchronous) */
int chr_selftest_sample_cdf(uint32_t n, const uint32_t *d_states, uint32_t nslots, int32_t ncdf,
                            const float *d_cdf_x, const float *d_cdf_y, float x0, float delta,
                            int32_t uniform_grid, float *d_out, void *stream);

/* ------------------------------------------------------------- device profile
 * replaces: the CHROMA_DEVICE_PROFILE build (chroma/cuda/profile.h:9-37) and
 * chroma.gpu.profiler.device_fetch / device_reset / device_report
 * (chroma/gpu/profiler.py:207-288).  Region counters (calls, cycles) of the split
 * step kernels, compiled only into libchroma_amd_prof.so (-DCHR_DEVICE_PROFILE=1;
 * chroma.gpu._native loads it when $CHROMA_DEVICE_PROFILE is set).  cycles are
 * lane-cycles of the shader clock (s_memtime): per work-item, the wave's time spent in
 * the region while that work-item took part, summed over work-items -- the reference's
 * per-thread clock64 sums.  Regions 0-5 keep the reference's ids. */
enum {
    CHR_PROF_INTERSECT_MESH = 0,      /* trace_kernel walks: calls = walks, cycles = node + triangle steps */
    CHR_PROF_INTERSECT_NODE = 1,      /* trace_kernel node steps (8-child slab test + stack) */
    CHR_PROF_INTERSECT_TRIANGLE = 2,  /* trace_kernel triangle steps (incl. the reference leaf-box check) */
    CHR_PROF_INTERSECT_BOX = 3,       /* child boxes slab-tested (calls only: part of the node steps) */
    CHR_PROF_FILL_MATERIAL = 4,       /* shade_kernel finish_fill (normal, material, surface of the hit) */
    CHR_PROF_FILL_ANALYTIC = 5,       /* kept for the reference's id (no analytic solids here: 0) */
    CHR_PROF_TRACE_REFILL = 6,        /* trace_kernel: publishing results + fetching the next rays */
    CHR_PROF_TRACE_IDLE = 7,          /* trace_kernel: lanes without work while their wave steps */
    CHR_PROF_SHADE_PHYSICS = 8,       /* shade_kernel propagate_to_boundary / _at_surface / _at_boundary */
    CHR_PROF_SHADE_OTHER = 9,         /* shade_kernel: state fetch wait, write-back, masks */
    CHR_PROF_TAIL_WALK = 10,          /* propagate_tail_kernel: the wave-spread walks (calls = walks) */
    CHR_PROF_TAIL_PHYSICS = 11,       /* propagate_tail_kernel: finish_fill + physics of the steps */
    CHR_PROF_TAIL_OTHER = 12,         /* propagate_tail_kernel: photon load / write-back / waiting */
    CHR_PROF_TRACE_KERNEL = 13,       /* whole trace_kernel (calls = work-items) */
    CHR_PROF_SHADE_KERNEL = 14,       /* whole shade_kernel */
    CHR_PROF_TAIL_KERNEL = 15,        /* whole propagate_tail_kernel */
    CHR_PROF_TRACE_DRAIN = 16,        /* trace_kernel: a wave's last <= 8 walks, whole-wave (calls = walks) */
    /* the lone walker's wave-cycles per phase of its iterations (walk_lone, the default, has no
       separate fetch phase: its node / record loads are waited for inside EXPAND / TRIS): */
    CHR_PROF_LONE_REFILL = 17,        /* cursors refilled from the shared stack */
    CHR_PROF_LONE_FETCH = 18,         /* nodes + triangles loaded (issued and waited for) */
    CHR_PROF_LONE_EXPAND = 19,        /* children slab-tested, near child, pushes, triangle list */
    CHR_PROF_LONE_TRIS = 20,          /* triangles tested, nearest hit reduced */
    CHR_PROF_LONE_WALK = 21,          /* all of the above (calls = iterations) */
    /* a long-lived photon's tail steps (its steps beyond the 64th), wave cycles per phase: */
    CHR_PROF_LONG_WALK = 22,          /* the walk (calls = such steps) */
    CHR_PROF_LONG_FILL = 23,          /* finish_fill: the hit's record, normal, material, surface */
    CHR_PROF_LONG_TO_BOUNDARY = 24,   /* propagate_to_boundary */
    CHR_PROF_LONG_AT_BOUNDARY = 25,   /* propagate_at_surface / _at_boundary */
    CHR_PROF_LONG_OTHER = 26,         /* the rest of the step: the kernel's loop, ballots, the walk's set-up */
    CHR_PROF_NREGIONS = 27,
    CHR_PROF_COUNT = 64               /* counter array length (profile.h:16) */
};
/* 1 when this library was built with the device profile, else 0 */
int chr_device_profile_enabled(void);
/* zero the counters (replaces the chroma_prof_reset kernel); CHR_ERR_INVALID without the profile build */
int chr_device_profile_reset(void *stream);
/* copy n <= CHR_PROF_COUNT counters to host arrays and the shader clock (kHz) the
 * cycles convert with (hipDeviceAttributeClockRate); synchronises the device */
int chr_device_profile_fetch(uint64_t *h_calls, uint64_t *h_cycles, int32_t n, uint32_t *clock_khz);
/* Photon watch (diagnostics, profile build only; no reference counterpart):
 * every step of photon `photon` (its index in a batch's arrays; d_pos_array =
 * that batch's pos array, NULL: any batch) run by the shade or tail kernels is
 * recorded as 20 words -- kind (1 shade, 2 tail), queue position, hit triangle,
 * walk distance, pos in (3), dir in (3), last hit in, material1, absorption and
 * scattering lengths, pos out (3), history out, time out, RNG slot (the layout
 * of the oracle's orc_set_watch).  chr_watch_set clears the record count;
 * chr_watch_fetch copies min(count, max_records, 4096) records and the count. */
int chr_watch_set(uint32_t photon, const float *d_pos_array);
int chr_watch_fetch(uint32_t *h_out, uint32_t max_records, uint32_t *nrecords);
/* The walk of one ray by trace_kernel (profile build): h_origin non-NULL arms the
 * log for the ray with exactly this origin (3 floats); with h_origin NULL,
 * copies min(count, max_events, 8192) 8-word events (kind 1 start, 2 pop,
 * 3 node expansion, 4 triangle fetched, 5 triangle hit, 6 leaf-box check,
 * 7 drain, 8 drain publish, 9 publish) and the count. */
int chr_watch_ray(const float *h_origin, uint32_t *h_events, uint32_t max_events, uint32_t *nevents);

/* ------------------------------------------------------------- misc */
const char *chr_last_error(void);
int chr_version(void);
/* sha256 (16 hex) of the sources this library was built from (tools/source_sha.py:
 * csrc/ and include/), compiled in by the Makefile; bench.py compares it with the
 * tree's own (so_source_sha vs kernel_source_sha) */
const char *chr_source_sha(void);

#ifdef __cplusplus
}
#endif
#endif /* CHROMA_AMD_H */
