/*
 * grt_api.h — C ABI of the MI355X-native geodesic ray tracer (gr_raytracer_amd).
 *
 * This is the drop-in boundary for the hot path of mdreem/gr_raytracer:
 *
 *   Raytracer::render_section_to_cie_buffer_raw   (src/rendering/raytracer.rs:195-244)
 *   Raytracer::supersample                         (src/rendering/raytracer.rs:320-384)
 *     -> Scene::color_of_ray                       (src/rendering/scene.rs:114-220)
 *        -> Integrator::integrate / rkf45          (src/rendering/integrator.rs:78-268,
 *                                                   src/rendering/runge_kutta.rs:86-182)
 *        -> Objects::intersects (Sphere / Disc)    (src/scene_objects/objects.rs:65-120)
 *        -> redshift / texture / blend shade       (src/rendering/{redshift,texture,color}.rs)
 *
 * The reference binds these through Rust traits (`RenderableGeometry`, `Geometry`,
 * `GeodesicSolver`, `Hittable`, `TextureMap`, `TemperatureComputer`); see
 * src/geometry/geometry.rs:15-153.  Here the scene is flattened to a plain-old-data
 * descriptor (grt_scene_desc) built once per frame on the host (camera tetrad and
 * look-up tables included, exactly like `create_scene`, src/cli/shared.rs:131-321),
 * and the per-pixel work runs in hand-written HIP kernels for gfx950.
 *
 * All signatures use plain C types only.  Every function returns 0 on success or a
 * negative errno-style code; grt_last_error() returns the text of the last failure
 * on the calling thread.
 */
#ifndef GRT_API_H
#define GRT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRT_ABI_VERSION 3

/* ---- enums (values are part of the ABI) -------------------------------------- */

/* configuration.rs:111-129 GeometryType. */
enum grt_geometry_kind {
  GRT_GEOM_EUCLIDEAN = 0,     /* geometry/euclidean.rs, Cartesian chart, (+,-,-,-)   */
  GRT_GEOM_SCHWARZSCHILD = 1, /* geometry/schwarzschild.rs, spherical chart, (+,-,-,-) */
  GRT_GEOM_KERR = 2,          /* geometry/kerr.rs, Kerr-Schild Cartesian, (-,+,+,+)   */
  GRT_GEOM_KERR_BL = 3,       /* geometry/kerr_bl.rs, Boyer-Lindquist, (-,+,+,+)      */
  GRT_GEOM_EUCLIDEAN_SPHERICAL = 4 /* geometry/euclidean_spherical.rs, flat space in the
                                      spherical chart, (+,-,-,-)                        */
};

/* configuration.rs:162-177 TextureConfig. */
enum grt_texture_kind {
  GRT_TEX_BITMAP = 0,   /* texture.rs:41-102  TextureMapper (bilinear)           */
  GRT_TEX_CHECKER = 1,  /* texture.rs:212-257 CheckerMapper                      */
  GRT_TEX_BLACKBODY = 2 /* texture.rs:104-210 BlackBodyMapper (LUT over log10 T) */
};

/* configuration.rs:188-219 ObjectsConfig. */
enum grt_object_kind {
  GRT_OBJ_SPHERE = 0,          /* scene_objects/sphere.rs                           */
  GRT_OBJ_DISC = 1,            /* scene_objects/disc.rs                             */
  GRT_OBJ_VOLUMETRIC_DISC = 2  /* scene_objects/volumetric_disc.rs (Perlin fBm gas,
                                  constant-step raymarch per intersection)          */
};

/* rendering/temperature.rs: ConstantTemperatureComputer / KerrTemperatureComputer. */
enum grt_temperature_kind {
  GRT_TEMP_CONSTANT = 0,
  GRT_TEMP_KERR_LUT = 1
};

/* scene.rs:25-30 RayClass. */
enum grt_ray_class { GRT_CLASS_ESCAPED = 0, GRT_CLASS_CAPTURED = 1, GRT_CLASS_HIT = 2 };

/* color.rs:16-21 ToneMappingMethod. */
enum grt_tone_mapping { GRT_TONE_REINHARD = 0, GRT_TONE_GLOBAL_LINEAR = 1 };

/* Per-pixel status: which RaytracerError (raytracer.rs:20-52) aborted the pixel.
 * A pixel with a non-zero status keeps the reference default {(0,0,0,1), Escaped}
 * (raytracer.rs:204-210, :232-239).  Bit 7 flags are informational. */
enum grt_status {
  GRT_OK = 0,
  GRT_ERR_MAX_STEPS_REACHED = 1,     /* runge_kutta.rs:179-181 (100 retries)           */
  GRT_ERR_NO_CIRCULAR_ORBIT = 2,     /* circular_orbit.rs:93-101                        */
  GRT_ERR_BELOW_RISCO = 3,           /* temperature.rs:204-217                          */
  GRT_ERR_NON_FINITE_RADIUS = 4,     /* temperature.rs:199-202                          */
  GRT_FLAG_HIT_OVERFLOW = 0x80       /* the device hit pool was full: this ray's candidates
                                        past GRT_MAX_HITS are missing.  The *_async
                                        calls return it (grt_hit_pool_reserve, then trace
                                        again); the synchronous calls trace the flagged
                                        pixels again, growing the pool to their need, and
                                        return it only past 2^31 - 1 records.            */
};

/* Stop reason of the integration (integrator.rs:22-27), recorded per pixel. */
enum grt_stop_reason {
  GRT_STOP_NONE = 0, /* step budget exhausted, no terminal event */
  GRT_STOP_HORIZON = 1,
  GRT_STOP_CELESTIAL = 2,
  GRT_STOP_NAN = 3,
  GRT_STOP_CLOSED_ORBIT = 4
};

#define GRT_MAX_OBJECTS 8
/* Window candidates a ray keeps in its fixed workspace slots; any further ones go to a
 * device-wide hit pool, so every window's intersection reaches the pixel as in the
 * reference (scene.rs:139-152, :206-210).  An implementation constant, not a limit. */
#define GRT_MAX_HITS 16

/* ---- POD scene descriptor ------------------------------------------------------ */

typedef struct grt_texture_desc {
  int32_t kind;            /* grt_texture_kind */
  int32_t _pad;
  double beaming_exponent; /* apply_beaming exponent (color.rs:72-80)              */
  /* GRT_TEX_BITMAP: caller-owned RGBA8 texels, row-major, width*height*4 bytes.    */
  const uint8_t* rgba;
  uint32_t width, height;
  /* GRT_TEX_CHECKER: cell counts and the two colours already in CIE XYZA          */
  double checker_width, checker_height;
  double c1[4], c2[4];
} grt_texture_desc;

typedef struct grt_object_desc {
  int32_t kind;          /* grt_object_kind */
  int32_t temp_kind;     /* grt_temperature_kind (Disc only)                       */
  /* Sphere: radius, Cartesian centre, constant temperature (sphere.rs:14-35).     */
  double radius;
  double center[3];
  double temperature;
  /* Disc: annulus in the z = 0 plane (disc.rs:335-356).                            */
  double inner_radius, outer_radius;
  /* Disc temperature model: constant, or the KerrTemperatureComputer LUT
   * (temperature.rs:29-118): r_isco, and n (r, T) pairs strictly increasing in r. */
  double temp_constant;
  double r_isco;
  const double* lut_r;
  const double* lut_t;
  uint32_t lut_n;
  uint32_t _pad2;
  grt_texture_desc texture;
  /* GRT_OBJ_VOLUMETRIC_DISC (volumetric_disc.rs:21-95, configuration.rs:200-217).
   * inner/outer radius, the temperature model and the texture are the Disc fields
   * above (cli/shared.rs:219-307 builds it like a Disc).  The axis is the configured
   * one, (0,0,1) when absent; grt_scene_create normalises it and derives e1, e2
   * exactly as VolumetricDisc::new (:61-73) and the Perlin permutation table from
   * perlin_seed (noise 0.9.0 PermutationTable::new, see grt_perlin_permutation). */
  double axis[3];
  double thickness;                        /* Gaussian sigma; capture slab 3x this  */
  double march_step_size;                  /* raymarch step (config step_size)      */
  double density_multiplier;
  double brightness_reference_temperature;
  double absorption, scattering;           /* sigma_a, sigma_s                      */
  double noise_scale[3];
  double noise_offset;
  uint64_t march_max_steps;                /* raymarch samples per intersection     */
  uint32_t num_octaves;
  uint32_t perlin_seed;                    /* config perlin_seed, default 1         */
} grt_object_desc;

/* The camera after Camera::new (camera.rs:151-196): position and velocity in the
 * geometry's native chart, the rotated + Lorentz-boosted tetrad rows t, x, y, z,
 * and the scalars used by get_direction_for (camera.rs:214-232). */
typedef struct grt_camera_desc {
  double position[4];
  double velocity[4];
  double tetrad[4][4];       /* tetrad[0]=e_t, [1]=e_x, [2]=e_y, [3]=e_z (components) */
  double alpha;              /* vertical field of view (pi/4 for the CLI, shared.rs:162) */
  double tan_half_alpha;     /* tan(alpha/2), host libm                                  */
  int64_t rows, cols;
  double spatial_signature;  /* signature[3]                                             */
  double spatial_handedness; /* camera.rs:134-148                                        */
  /* sin/cos of the camera's polar angle (position[2]) for the spherical and BL charts,
   * evaluated once on the host (libm) like every other per-frame constant.            */
  double sin_theta, cos_theta;
} grt_camera_desc;

typedef struct grt_scene_desc {
  uint32_t abi_version;      /* = GRT_ABI_VERSION */
  int32_t geometry;          /* grt_geometry_kind */
  double radius;             /* r_s (Schwarzschild radius)                      */
  double a;                  /* spin parameter (Kerr, KerrBL)                   */
  double horizon_epsilon;
  /* IntegrationConfiguration (integrator.rs:46-67), from GlobalOpts (cli.rs:5-47). */
  uint64_t max_steps;
  double max_radius;
  double step_size;
  double epsilon;
  grt_camera_desc camera;
  grt_texture_desc celestial;
  double celestial_temperature;
  uint32_t n_objects;        /* <= GRT_MAX_OBJECTS, tested in config order     */
  uint32_t _pad;
  grt_object_desc objects[GRT_MAX_OBJECTS];
  /* BlackBodyMapper LUT (texture.rs:120-138): n entries of (log10 T, X, Y, Z).    */
  const double* bb_log_t;
  const double* bb_xyz;      /* 3*n, interleaved X,Y,Z                          */
  uint32_t bb_n;
  uint32_t _pad3;
  /* Inverse sRGB companding (color.rs:301-308) of the 256 8-bit codes.            */
  double srgb_to_linear[256];
  /* AdaptiveSamplingConfig.object_hit_opacity_threshold (configuration.rs:36).    */
  double object_hit_opacity_threshold;
} grt_scene_desc;

/* ---- host-side scene setup (the Rust host's create_scene, cli/shared.rs) -------- */

/* GlobalOpts (cli.rs:5-47). */
typedef struct grt_global_opts {
  int64_t width, height;
  double step_size;
  uint64_t max_steps;
  double max_radius;
  double epsilon;
  double camera_position[3];
  double phi, theta, psi;
  int32_t tone_mapping;       /* 0 Reinhard, 1 GlobalLinear (color.rs:16-21) */
  int32_t show_sampling_mask;
  uint8_t sampling_mask_color[3];
  uint8_t _pad[5];
} grt_global_opts;

/* AdaptiveSamplingConfig (configuration.rs:21-94). */
typedef struct grt_adaptive_config {
  int32_t enabled;
  uint32_t samples_per_axis;
  double luminance_contrast_threshold;
  double opacity_contrast_threshold;
  int32_t has_minimum_luminance;
  int32_t exclude_background_contrast;
  double minimum_luminance;
  double object_hit_opacity_threshold;
} grt_adaptive_config;

typedef struct grt_host_scene grt_host_scene; /* owns textures + LUTs + desc */

void grt_default_global_opts(grt_global_opts* opts);
void grt_default_adaptive_config(grt_adaptive_config* cfg);

/* Parse a scene TOML (configuration.rs schema) and build the frame exactly like
 * `main.rs:80-116` + `cli/<geometry>.rs::create_scene_internal` + `create_scene`.
 * Texture paths are resolved relative to `resource_root` (NULL = cwd). */
int grt_host_scene_load(const char* toml_path, const char* resource_root,
                        const grt_global_opts* opts, grt_host_scene** out);
/* Geometry and integration configuration only (no camera, textures or objects): what
 * `render-ray-at` uses (main.rs:143-168 builds the geometry, not a scene). */
int grt_host_geometry_load(const char* toml_path, const grt_global_opts* opts,
                           grt_host_scene** out);
const grt_scene_desc* grt_host_scene_desc(const grt_host_scene* s);
/* The camera grt_host_scene_load would have built for this scene had its options carried
 * these --camera-position / --phi / --theta / --psi values: the chart conversion, the
 * TOML's camera_velocity mode (StaticObserver, Zamo, Explicit), the future-directed check
 * and grt_camera_build with the scene's rows and cols.  Byte for byte the `camera` of
 * such a load's descriptor; the same errors (-EINVAL, grt_last_error) where that load
 * fails on the camera.  The cameras of grt_render_sequence. */
int grt_host_scene_camera(const grt_host_scene* s, const double position[3], double phi, double theta,
                          double psi, grt_camera_desc* out);
/* The info-level lines the reference logs while it builds this scene, one per line, in
 * order (today the temperature LUT's, KerrTemperatureComputer::new, temperature.rs:55-102:
 * the r_isco clamp, "Computed r_isco: ...", "Max f: ...", "Computed m_dot: ..."; numbers
 * in Rust's f64 Display form).  Owned by the scene; "" when there are none. */
const char* grt_host_scene_log(const grt_host_scene* s);
void grt_host_scene_adaptive(const grt_host_scene* s, grt_adaptive_config* out);
int grt_host_scene_destroy(grt_host_scene* s);

/* Camera::new (camera.rs:151-196) for an explicit position/velocity in the native
 * chart of `geometry` (radius, a as in grt_scene_desc).  Fails with -EDOM when a
 * tetrad is not orthonormal (TetradValidator, tetrad.rs:60-131). */
int grt_camera_build(int32_t geometry, double radius, double a,
                     const double position[4], const double velocity[4], double alpha,
                     int64_t rows, int64_t cols, double phi, double theta, double psi,
                     grt_camera_desc* out);

/* Per-geometry support quantities used by the host to place the camera. */
int grt_stationary_velocity(int32_t geometry, double radius, double a,
                            const double position[4], double out[4]);
int grt_zamo_velocity(int32_t geometry, double radius, double a,
                      const double position[4], double out[4]);
/* Chart conversions (spherical_coordinates_helper.rs:5-61). */
void grt_cartesian_to_spherical(const double in[4], double out[4]);
void grt_cartesian_to_boyer_lindquist(double a, const double in[4], double out[4]);

/* KerrTemperatureComputer::new (temperature.rs:45-118): fills n (r, T) pairs.
 * Returns -ERANGE on DenominatorCloseToZero / NoCircularOrbitPossible. */
int grt_kerr_temperature_lut(double temperature, double outer_radius, double a,
                             double radius, uint32_t n, double* lut_r, double* lut_t,
                             double* r_isco);
double grt_r_isco(double radius, double a);
/* BlackBodyMapper::new (texture.rs:121-138): n entries of (log10 T, XYZ). */
int grt_blackbody_lut(uint32_t n, double* log_t, double* xyz);
/* integrate_blackbody_xyz (black_body_radiation.rs:18-41). */
void grt_blackbody_xyz(double temperature, double redshift, double out_xyz[3]);
/* srgb_to_xyz (color.rs:310-332), alpha := a/255 (CIETristimulus::from_color). */
void grt_srgb_to_xyza(uint8_t r, uint8_t g, uint8_t b, uint8_t a, double out[4]);
/* Perlin::new(seed) of the `noise` crate 0.9.0 (volumetric_disc.rs:83), restated from
 * its published source (the crate is not vendored): PermutationTable::new seeds
 * rand_xorshift 0.3's XorShiftRng with the words [1, seed, seed, seed] and shuffles
 * 0..=255 with rand 0.8's SliceRandom::shuffle (Fisher-Yates, gen_range by widening
 * multiply + rejection).  out[i] = values[i]. */
void grt_perlin_permutation(uint32_t seed, uint8_t out[256]);
/* VolumetricDisc::new's frame (volumetric_disc.rs:61-73): the normalised axis
 * ((0,0,1) when |axis|^2 <= f64::EPSILON) and the in-plane unit vectors e1, e2. */
void grt_volumetric_frame(const double axis_in[3], double axis[3], double e1[3], double e2[3]);
/* xyz_to_srgb (color.rs:225-241): one XYZ colour -> sRGB8, linear * exposure, no
 * tone mapping (the `blackbody` subcommand, cli/blackbody.rs:7-25). */
void grt_xyz_to_srgb(const double xyz[3], double exposure, uint8_t rgb_out[3]);
/* run_blackbody_spectrum (cli/blackbody.rs:27-95): width x height RGBA8 image of
 * integrate_blackbody_xyz(T, z), T linear in x over [min, max] temperature, z linear
 * in y over [min, max] redshift, tone-mapped like a render (exposure 1), alpha 255. */
int grt_blackbody_spectrum(double min_temperature, double max_temperature, double min_redshift,
                           double max_redshift, uint32_t width, uint32_t height,
                           int32_t tone_mapping, uint8_t* rgba_out);
/* xyz -> tone-mapped sRGB8 (color.rs:204-298), whole buffer = grt_linear_max (only for
 * GlobalLinear) + grt_tonemap.  Split so that a frame spread over several processes
 * can reduce the three channel maxima (MAX) before mapping its own rows. */
void grt_linear_max(const double* xyza, size_t n, double exposure, double max3[3]);
int grt_tonemap(const double* xyza, size_t n, int32_t tone_mapping, double exposure,
                const double max3[3], uint8_t* rgb_out);
int grt_xyz_to_srgb8(const double* xyza, size_t n, int32_t tone_mapping, double exposure,
                     uint8_t* rgb_out);

/* ---- device hot path -------------------------------------------------------- */

typedef struct grt_scene grt_scene; /* device-resident copy, one per GPU on demand */

typedef struct grt_stats {
  uint64_t accepted_steps; /* iterations of integrator.rs:100 that produced a step     */
  uint64_t attempts;       /* rkf45_step evaluations (6 RHS each)                      */
  uint64_t rays;
  uint64_t hit_overflows;  /* pixels flagged GRT_FLAG_HIT_OVERFLOW: for the synchronous calls
                              0 unless the pool would need more than 2^31 - 1 records     */
  double kernel_ms;        /* hipEvent time of the integration kernel(s)               */
  /* VolumetricDisc raymarches (volumetric_disc.rs:199-328): one per window-nearest
   * volumetric intersection whose colour reaches the composite, and their samples. */
  uint64_t march_jobs;
  uint64_t march_samples;
  uint64_t march_noise_samples; /* samples inside the density's support (fBm evaluated) */
  uint64_t march_emit_samples;  /* samples with density > 0 that emitted                */
} grt_stats;

/* Optional per-sample sub-pixel offsets (get_ray_for_offset, camera.rs:247-254):
 * sample k traces pixel (row0 + pix[k] / cols, col0 + pix[k] % cols) at (dx[k], dy[k]). */
typedef struct grt_offsets {
  uint64_t count;
  const uint32_t* pixel_index;
  const double* dx;
  const double* dy;
} grt_offsets;

/* Optional extra per-sample outputs for parity work (any pointer may be NULL). */
typedef struct grt_aux_out {
  double* xyza64;       /* 4 doubles per sample: the f64 colour before the f32 cast   */
  uint32_t* steps;      /* accepted steps per sample                                  */
  uint8_t* stop_reason; /* grt_stop_reason per sample                                 */
  uint32_t* hits;       /* windows with an intersection per sample: intersections.len()
                           of scene.rs:141-152 before the terminal colour (for a pixel
                           aborted by a window error, the windows before it)           */
} grt_aux_out;

int grt_scene_create(const grt_scene_desc* desc, grt_scene** out);
int grt_scene_destroy(grt_scene* scene);
const char* grt_last_error(void);
int grt_device_count(void);
/* SHA-256 (64 hex digits) of the sources this library was built from
 * (gr_raytracer_amd/source_hash.py; "unstamped" for a copy built outside the checkout).
 * No reference counterpart: it ties a prebuilt library to its checkout. */
const char* grt_source_hash(void);

/* Trace a rows x cols rectangle at 1 spp (or the offset list) on `device`.
 * Host output arrays, row-major over the rectangle (or per offset entry). */
int grt_render_pixels(grt_scene* scene, int device, uint32_t row0, uint32_t col0,
                      uint32_t rows, uint32_t cols, const grt_offsets* offsets,
                      float* xyza_out, uint8_t* class_out, uint8_t* status_out,
                      const grt_aux_out* aux, grt_stats* stats);

/* Same, but every output pointer is a DEVICE pointer on `device` and the work is
 * enqueued on `stream` (a hipStream_t, NULL = default stream) without a host sync.
 * `device_stats` is a device buffer of 4 uint64 counters (accepted, attempts, rays,
 * overflows) that the kernel accumulates into (caller zeroes it). */
int grt_render_pixels_async(grt_scene* scene, int device, void* stream,
                            uint32_t row0, uint32_t col0, uint32_t rows, uint32_t cols,
                            float* d_xyza, uint8_t* d_class, uint8_t* d_status,
                            double* d_xyza64, uint32_t* d_steps, uint8_t* d_stop,
                            uint64_t* d_stats);

/* Whole section with the reference's adaptive supersampling
 * (render_section_to_cie_buffer[_supersampled], raytracer.rs:177-318), fully on the
 * device: 1-spp pass, exact 99th-percentile floor, 8-neighbour selection, 16 jittered
 * rays per selected pixel, ordered average.  Output: f64 XYZA per pixel. */
int grt_render_section(grt_scene* scene, int device, uint32_t from_row, uint32_t from_col,
                       uint32_t to_row, uint32_t to_col, const grt_adaptive_config* cfg,
                       const double* sampling_mask_xyza, double* xyza_out,
                       uint8_t* class_out, uint64_t* n_supersampled, grt_stats* stats,
                       uint8_t* status_out /* nullable: grt_status of each pixel's 1-spp ray, the
                                              error the reference logs at raytracer.rs:232-239 */);

/* Failed sub-samples of the supersample pass (supersample's Err arm, raytracer.rs:357-362,
 * which the reference logs as "Unable to compute color for ray at pixel (col, row)").
 * The caller provides `capacity` entries; `count` returns how many failed (it may exceed
 * the capacity).  Entries are sorted by (pixel, sample). */
typedef struct grt_subsample_failures {
  uint64_t capacity;
  uint32_t* pixel;   /* pixel index, row-major in the section (shard: in the frame)      */
  uint32_t* sample;  /* nullable: stratum index stratum_row * spa + stratum_col          */
  uint8_t* status;   /* grt_status of the failed sub-sample ray                         */
  uint64_t count;    /* out                                                             */
  /* Nullable.  When set, the list also holds the sub-rays that ended without an error
   * but on NaN coordinates or without a terminal event (status 0, stop GRT_STOP_NAN /
   * GRT_STOP_NONE), which the reference logs from color_of_ray (scene.rs:178-183,
   * :196-202); every entry then carries its stop reason and accepted steps.          */
  uint8_t* stop;
  uint32_t* steps;   /* nullable */
} grt_subsample_failures;

/* grt_render_section plus the failed sub-samples (nullable) and the 1-spp rays' stop
 * reasons and accepted steps per section pixel (nullable; the reference's color_of_ray
 * logs the NaN and no-terminal-event rays, scene.rs:178-183, :196-202).  The whole
 * section stays on the device between the 1-spp pass and the supersample pass: the
 * luminance floor, the selection, its compaction and count, and the sub-ray launches'
 * sizes are decided there (no host round trip). */
int grt_render_section_ex(grt_scene* scene, int device, uint32_t from_row, uint32_t from_col,
                          uint32_t to_row, uint32_t to_col, const grt_adaptive_config* cfg,
                          const double* sampling_mask_xyza, double* xyza_out, uint8_t* class_out,
                          uint64_t* n_supersampled, grt_stats* stats, uint8_t* status_out,
                          grt_subsample_failures* failures, uint8_t* stop_out, uint32_t* steps_out);

/* Row-band sharding of one frame across GPUs (multi-GPU render).
 * The frame's rows are cut into bands of `band_rows` rows (the last may be short);
 * shard s of n owns the bands b with b % n == s.  Its output is the full-width rows of
 * those bands, packed in increasing frame order ("local rows").  Cyclic bands balance
 * the cost, which is concentrated around the shadow and the disc.  The reference has
 * one process rendering everything (raytracer.rs:195-244); the per-pixel results of a
 * shard are identical to rendering the same rows through grt_render_pixels. */
typedef struct grt_row_shard {
  uint32_t band_rows; /* >= 1; a multiple of 8 keeps the 8x8 pixel tiles inside a band */
  uint32_t shard;     /* < n_shards */
  uint32_t n_shards;  /* >= 1 */
} grt_row_shard;

/* Number of local rows of shard `sh` in a frame of `frame_rows` rows. */
uint32_t grt_shard_row_count(uint32_t frame_rows, const grt_row_shard* sh);
/* Frame row of local row `local_row` of shard `sh`. */
uint32_t grt_shard_frame_row(uint32_t local_row, const grt_row_shard* sh);

/* Trace all local rows of a shard (full frame width) at 1 spp: host outputs,
 * local-row-major, like grt_render_pixels. */
int grt_render_shard(grt_scene* scene, int device, const grt_row_shard* sh, float* xyza_out,
                     uint8_t* class_out, uint8_t* status_out, const grt_aux_out* aux,
                     grt_stats* stats);
/* Same with device outputs on `stream`, like grt_render_pixels_async. */
int grt_render_shard_async(grt_scene* scene, int device, void* stream, const grt_row_shard* sh,
                           float* d_xyza, uint8_t* d_class, uint8_t* d_status, double* d_xyza64,
                           uint32_t* d_steps, uint8_t* d_stop, uint64_t* d_stats);

/* ---- one frame across several GPUs of this process (north_star) ----
 * The north-star layout behind the C ABI: the frame's rows in cyclic bands of band_rows
 * (band b -> devices[b % n_devices], grt_row_shard), one host thread per device tracing
 * its bands (grt_render_shard_async), and ONE RCCL gather (grouped send / receive over
 * xGMI, one communicator per device from ncclCommInitAll) of every device's pixel records
 * to devices[0], where a kernel de-interleaves them into frame order.  With supersampling
 * (cfg->enabled, or a sampling mask) one RCCL allgather of each pixel's (Y, alpha, class)
 * (17 B) comes first: the selection stencil reads neighbours in other devices' bands and
 * the luminance floor is a percentile of the whole frame; each device then supersamples
 * its own pixels (grt_supersample_shard_device).  Replaces the single-process frame
 * driver of the `render` command: render_section_to_cie_buffer[_raw|_supersampled]
 * (raytracer.rs:195-318) as Raytracer::render_section calls it (:460-497, main.rs:80-116).
 * Every pixel equals grt_render_pixels / grt_render_section_ex of the same frame on one
 * device.  The communicators, streams and device scratch are created on the first call
 * for a device list and kept (grt_multi_release frees them).
 *
 * Transports (grt_set_multi_transport, process-wide like grt_set_arithmetic, read once per
 * grt_render_frame_multi call; default GRT_TRANSPORT_RCCL, the path above):
 *  - GRT_TRANSPORT_PEER: no RCCL.  The devices are mapped into each other once per device
 *    list (hipDeviceEnablePeerAccess); after the host barrier that follows each rank's
 *    stream synchronise, a kernel on the reading device dereferences the owners' blocks in
 *    place (all ranks for the (Y, alpha, class) exchange, devices[0] for the final gather).
 *    A list with a device pair that cannot be mapped runs GRT_TRANSPORT_PEER_STAGED
 *    (grt_multi_report.transport says which ran).
 *  - GRT_TRANSPORT_PEER_STAGED: no RCCL and no mapping.  hipMemcpyPeerAsync copies each
 *    block into the reader's staging, then the de-interleave kernel of the RCCL path.
 * Neither loads librccl or creates a communicator, at n_devices = 1 too.  Under both, a
 * device list may name one ordinal several times: each entry is a rank with its own
 * stream, events and scratch ("virtual ranks"; {0, 0, 0} is three ranks on GPU 0), which is
 * how the N > 1 host path is held to the single-device frame bit for bit on one GPU
 * (tests/test_multi_peer.py).  Under GRT_TRANSPORT_RCCL a repeated ordinal is -EINVAL.  No
 * N > 1 frame over distinct GPUs has run on hardware under any transport.  A failure on
 * one rank ends the frame on all of them ("rank k (device d): ..."); the cached state
 * stays usable. */
#define GRT_MULTI_MAX_DEVICES 16

enum grt_multi_transport { GRT_TRANSPORT_RCCL = 0, GRT_TRANSPORT_PEER = 1, GRT_TRANSPORT_PEER_STAGED = 2 };
/* 0 on success, -EINVAL for a mode that is none of the above. */
int grt_set_multi_transport(int mode);
int grt_get_multi_transport(void);

/* Host outputs in frame order (camera rows x cols); a NULL field is not gathered.  The
 * gather moves 2 B per pixel (class, status) plus the requested fields: f32 XYZA + class
 * + status is the 18-B pixel record of the 1-spp frame. */
typedef struct grt_frame_out {
  float* xyza;         /* f32 XYZA (1-spp frames only: NULL with supersampling)          */
  double* xyza64;      /* f64 XYZA, the supersampled colour where selected (required with
                          supersampling)                                                  */
  uint8_t* ray_class;  /* RayClass of the 1-spp ray                                       */
  uint8_t* status;     /* grt_status of the 1-spp ray (raytracer.rs:232-239)              */
  uint8_t* stop;       /* grt_stop_reason of the 1-spp ray                                */
  uint32_t* steps;     /* accepted steps of the 1-spp ray                                 */
} grt_frame_out;

typedef struct grt_multi_report {
  uint32_t n_devices;
  uint32_t record_bytes;     /* bytes per pixel the gather moved                                */
  uint32_t attempts;         /* traces of the frame (more than 1 when a hit pool had to grow)   */
  uint32_t transport;        /* the grt_multi_transport that ran                                */
  double wall_ms;            /* the whole call, host clock                                      */
  double gather_ms;          /* last trace: gather + de-interleave on devices[0] (events)       */
  double allgather_ms;       /* supersampling: the (Y, alpha, class) allgather, max over devices */
  double trace_ms[GRT_MULTI_MAX_DEVICES];        /* per device: its trace (+ supersample pass)   */
  uint64_t accepted_steps[GRT_MULTI_MAX_DEVICES];
  uint64_t rows[GRT_MULTI_MAX_DEVICES];          /* frame rows each device traced                */
} grt_multi_report;

/* Render the whole camera frame over n_devices GPUs (1 <= n <= 16; distinct under
 * GRT_TRANSPORT_RCCL, where n = 1 runs the same RCCL path with a one-rank communicator).  cfg (nullable): the scene's adaptive
 * configuration (grt_host_scene_adaptive), NULL or !enabled = 1 spp; sampling_mask_xyza
 * (nullable): paint the selected pixels instead (--show-sampling-mask).  stats: summed
 * counters, kernel_ms the slowest device's trace.  failures (nullable): every device's
 * failed sub-samples, frame pixel indices, sorted by (pixel, sample).  A trace that lost
 * hit candidates grows the pools and traces the frame again (at most 3 traces; after
 * that the pixels keep GRT_FLAG_HIT_OVERFLOW and stats->hit_overflows counts them). */
int grt_render_frame_multi(grt_scene* scene, int n_devices, const int* devices, uint32_t band_rows,
                           const grt_adaptive_config* cfg, const double* sampling_mask_xyza,
                           const grt_frame_out* out, uint64_t* n_supersampled, grt_stats* stats,
                           grt_subsample_failures* failures, grt_multi_report* report);
/* Free the communicators, streams and scratch grt_render_frame_multi keeps (no frame may
 * be in flight). */
void grt_multi_release(void);

/* ---- camera sequences: K cameras over one resident scene ------------------------------
 * An animation along a camera path changes nothing of the scene but the camera, so the
 * frames share the scene's device copy (textures, LUTs, workspace) and are traced stacked:
 * K frames of rows x cols as one rectangle of K * rows rows, one tile queue, each ray with
 * the camera of the frame its row lies in (geodesic_seq.hip).  Small frames that cannot
 * fill the GPU one by one then run side by side.  Every frame is bit-identical to
 * rendering its camera alone (grt_render_pixels / grt_render_section_ex on a scene created
 * with that camera): the operations are the same.
 * The sequence trace always runs the exact arithmetic: grt_set_arithmetic(1) does not
 * apply (there is no fused sequence unit).  grt_set_schedule, grt_set_two_ended and
 * grt_set_tail apply to the stacked rectangle as to any other (scheduling only). */
typedef struct grt_sequence_report {
  uint32_t n_frames;
  uint32_t n_launches;         /* launch groups = stacked 1-spp traces of whole frames       */
  uint32_t frames_per_launch;  /* frames in a full group (the last one may hold fewer)       */
  uint32_t _pad;
  double wall_ms;              /* the whole call, host clock                                 */
  double trace_ms;             /* summed event time of the stacked 1-spp traces (re-traces of
                                  pixels that overflowed the hit pool included)              */
  double supersample_ms;       /* summed event time of the per-frame selection and
                                  supersample passes                                         */
} grt_sequence_report;

/* Render n_cameras frames of `scene` on `device`.  Every camera must have the scene's rows
 * and cols (grt_host_scene_camera builds such cameras), else -EINVAL; only whole frames.
 * out: host arrays, frame-major [n_cameras][rows][cols], a NULL field is not written;
 * xyza is for 1 spp, xyza64 is required with supersampling (cfg->enabled or a mask; cfg
 * and sampling_mask_xyza as in grt_render_frame_multi).  n_supersampled and failures
 * (nullable): arrays of n_cameras, one per frame, each filled as grt_render_section_ex
 * fills its own.  stats (nullable): the counters of the whole call, kernel_ms =
 * trace_ms + supersample_ms.  Frames go to the device in launch groups
 * (grt_set_sequence_group); results are identical for every group size.  Pixels that
 * lost hit candidates (GRT_FLAG_HIT_OVERFLOW) are traced again with a grown pool as the
 * synchronous single-frame calls do. */
int grt_render_sequence(grt_scene* scene, int device, uint32_t n_cameras,
                        const grt_camera_desc* cameras, const grt_adaptive_config* cfg,
                        const double* sampling_mask_xyza, const grt_frame_out* out,
                        uint64_t* n_supersampled, grt_stats* stats,
                        grt_subsample_failures* failures, grt_sequence_report* report);
/* Rays per launch group of grt_render_sequence (0 = default 2^22: ~4.6 GB of workspace at
 * 64 B + 16 x 64 B per ray).  A group holds as many whole frames as fit, at least one.
 * Scheduling only.  Process-wide; read once per call. */
int grt_set_sequence_group(uint64_t rays);

/* ---- geometry buffer: trace a rectangle once, re-shade it many times --------------------
 * The integration depends on the geometry, the camera and the shapes of the objects; the
 * textures, beaming exponents, temperatures, the celestial sphere, the hit-opacity threshold
 * and the tone mapping play no part in it.  A geometry buffer ("g-buffer", the lensing map
 * of the rectangle) keeps what the shade pass reduces each 1-spp ray to before any of those
 * is applied (Scene::color_of_ray, scene.rs:141-219), so the rectangle can be shaded again
 * under any scene with the same shape key without integrating a geodesic.  Re-shading is
 * bit-identical to grt_render_pixels of the appearance scene with the traced camera and
 * integration parameters.  The reference has no counterpart.
 *
 * Per pixel, row-major over the rectangle:
 *   status, stop, steps   what grt_render_pixels returns (window errors included);
 *   sky_u, sky_v, sky_redshift
 *                         the arguments of the celestial sphere's texture lookup (1 - u, v,
 *                         redshift) for a pixel with status 0 that ended on it (stop =
 *                         GRT_STOP_CELESTIAL), +0.0 for every other pixel;
 *   layer_start           n_pixels + 1 entries: the exclusive prefix sum of the pixels' layer
 *                         counts; layer_start[n_pixels] = n_layers.
 * Per layer, pixel-major, front to back.  A layer is one window's nearest intersection,
 * the hits that enter the blend (grt_aux_out.hits counts them); a pixel whose status is not
 * 0 has none, and there is no cap per pixel:
 *   object                index into grt_scene_desc.objects;
 *   u, v, redshift        the arguments of the object's texture lookup;
 *   radius                the argument of the disc's temperature model; +0.0 for a sphere.
 *
 * The shape key is everything of a scene that decides hits, window errors and the recorded
 * numbers: geometry, radius, a, n_objects and per object kind, temp_kind, radius, center,
 * inner_radius, outer_radius, r_isco.  Textures, temperatures, LUT contents, the celestial
 * sphere, the hit threshold, the camera and the integration parameters are free to differ
 * between the traced scene and an appearance scene.
 *
 * The g-buffer trace always runs the exact arithmetic, whatever grt_set_arithmetic says (as
 * Kerr-Schild and the camera sequences do): re-shading reproduces the exact frame.  Scenes
 * with a GRT_OBJ_VOLUMETRIC_DISC are refused (-ENOTSUP): its colour is raymarched, not a
 * function of (u, v, redshift, temperature).  One rectangle on one device, at 1 spp or with
 * the adaptive pass's sub-rays (the sub-sample set below), or the whole frames of a camera
 * sequence, one buffer each (grt_gbuffer_trace_sequence below), or the whole frame at 1 spp
 * over several GPUs, assembled into one buffer on the first (grt_gbuffer_trace_multi below):
 * no offset lists, and no row shards as buffers of their own.
 * A grt_gbuffer is not synchronised: one host thread at a time per buffer. */
typedef struct grt_gbuffer grt_gbuffer; /* device-resident, owns its arrays */

typedef struct grt_gbuffer_object_shape {
  int32_t kind;       /* grt_object_kind */
  int32_t temp_kind;  /* grt_temperature_kind */
  double radius;
  double center[3];
  double inner_radius, outer_radius;
  double r_isco;
} grt_gbuffer_object_shape;

typedef struct grt_gbuffer_shape {
  int32_t geometry;   /* grt_geometry_kind */
  uint32_t n_objects;
  double radius, a;
  grt_gbuffer_object_shape objects[GRT_MAX_OBJECTS]; /* entries past n_objects are zero */
} grt_gbuffer_shape;

typedef struct grt_gbuffer_info {
  uint32_t row0, col0, rows, cols; /* the rectangle in the traced camera's frame */
  uint64_t n_pixels;               /* rows * cols */
  uint64_t n_layers;
  int32_t device;                  /* where the buffer lives (the traced device in a file) */
  uint32_t _pad;
  grt_gbuffer_shape shape;
  /* what was traced: never compared with an appearance scene, compared byte for byte with
   * the tracer of grt_gbuffer_supersample */
  grt_camera_desc camera;
  uint64_t max_steps;
  double max_radius, step_size, epsilon, horizon_epsilon;
} grt_gbuffer_info;

/* Host arrays of a g-buffer (caller-allocated; sizes from grt_gbuffer_info). */
typedef struct grt_gbuffer_arrays {
  uint8_t* status;       /* n_pixels */
  uint8_t* stop;         /* n_pixels */
  uint32_t* steps;       /* n_pixels */
  double* sky_u;         /* n_pixels */
  double* sky_v;         /* n_pixels */
  double* sky_redshift;  /* n_pixels */
  uint64_t* layer_start; /* n_pixels + 1 */
  uint8_t* object;       /* n_layers */
  double* u;             /* n_layers */
  double* v;             /* n_layers */
  double* redshift;      /* n_layers */
  double* radius;        /* n_layers */
} grt_gbuffer_arrays;

/* Trace rows x cols at (row0, col0) at 1 spp on `device` with the exact kernels and keep
 * its g-buffer.  A trace that lost hit candidates grows the hit pool to its need and traces
 * the rectangle again (at most 3 traces, else -ENOMEM): a g-buffer never holds a pixel
 * flagged GRT_FLAG_HIT_OVERFLOW.  stats (nullable): the counters of the traces,
 * kernel_ms their event time.  -EINVAL for an empty rectangle or one outside the frame,
 * -ENOTSUP for a scene with a VolumetricDisc. */
int grt_gbuffer_trace(grt_scene* scene, int device, uint32_t row0, uint32_t col0, uint32_t rows,
                      uint32_t cols, grt_gbuffer** out, grt_stats* stats);
/* Event times of grt_gbuffer_trace in ms: [0] the trace(s), [1] the layer scan and the
 * fill.  Zeros for an uploaded buffer. */
int grt_gbuffer_trace_times(const grt_gbuffer* gb, double ms[2]);
int grt_gbuffer_info_get(const grt_gbuffer* gb, grt_gbuffer_info* out);
/* Copy the arrays to the host (every pointer non-null, sized by grt_gbuffer_info_get). */
int grt_gbuffer_download(const grt_gbuffer* gb, const grt_gbuffer_arrays* host);
/* A device buffer on `device` from host arrays (info->device is ignored).  The arrays are
 * checked like a file's (grt_gbuffer_read_file): -EINVAL, never a crash. */
int grt_gbuffer_upload(const grt_gbuffer_info* info, const grt_gbuffer_arrays* host, int device,
                       grt_gbuffer** out);
/* Shade the buffer under `appearance` on the buffer's device (the scene's copy there,
 * created on demand): host outputs per pixel as grt_render_pixels writes them; xyza64
 * (4 f64 per pixel) and kernel_ms (event time of the shade kernel) are nullable.  -EINVAL
 * when the scene's shape key differs from the buffer's (grt_last_error names the field). */
int grt_gbuffer_shade(grt_scene* appearance, const grt_gbuffer* gb, float* xyza_out, uint8_t* class_out,
                      uint8_t* status_out, double* xyza64_out, float* kernel_ms);
int grt_gbuffer_destroy(grt_gbuffer* gb);

/* ---- The g-buffer of the whole frame, traced over several GPUs ----
 * grt_render_frame_multi's row bands (band b -> devices[b % n_devices]), one host thread per
 * rank with the streams, scratch and barrier of the same cached context: each rank traces
 * its own shard with the exact kernels and fills its part as grt_gbuffer_trace does (a rank
 * that loses hit candidates grows its own pool and traces its own shard again, at most 3
 * traces, else -ENOMEM), laid out as ONE block.  After a barrier, devices[0]'s allocations and a
 * second barrier (so that no rank enters the transport when any has failed) the blocks reach
 * devices[0] by the transport of grt_set_multi_transport (read once per call; a peer list
 * with a pair that cannot be mapped runs staged), where two kernels put the per-pixel arrays
 * into frame order, an exclusive sum of the layer counts gives the frame's layer_start, and
 * every layer moves to its place by its band.  The result is an ordinary grt_gbuffer of the
 * whole camera frame on devices[0]: its grt_gbuffer_info and all twelve arrays are byte for
 * byte those of grt_gbuffer_trace(scene, devices[0], 0, 0, rows, cols, ...), so every call
 * above and below works on it unchanged.  grt_gbuffer_trace_times: [0] the slowest rank's
 * trace, [1] the slowest rank's scan + fill plus gather_ms.  stats (nullable): summed as
 * grt_render_frame_multi sums them.
 * Device lists as grt_render_frame_multi's: 1..16 entries, an ordinal may repeat under the
 * peer transports (one rank per entry), a repeat under GRT_TRANSPORT_RCCL is -EINVAL, and so
 * is an ordinal the machine does not have.  -ENOTSUP for a scene with a VolumetricDisc,
 * -EINVAL for band_rows = 0 or a null scene, devices or out, -EOVERFLOW for a frame of more
 * than INT_MAX - 1 pixels: all before any launch.  On any failure *out is NULL and nothing
 * stays allocated outside the cached context; a failure on one rank ends the call on all
 * ("rank k (device d): ...").  No N > 1 frame over distinct GPUs has run on hardware under
 * any transport. */
typedef struct grt_gbuffer_multi_report {
  uint32_t n_devices, transport;                 /* the grt_multi_transport that ran */
  uint32_t n_traces[GRT_MULTI_MAX_DEVICES];      /* per rank; > 1 when its hit pool had to grow */
  uint64_t rows[GRT_MULTI_MAX_DEVICES];
  uint64_t layers[GRT_MULTI_MAX_DEVICES];        /* layers each rank filled */
  uint64_t block_bytes[GRT_MULTI_MAX_DEVICES];   /* what the gather moved from each rank */
  double trace_ms[GRT_MULTI_MAX_DEVICES], fill_ms[GRT_MULTI_MAX_DEVICES];
  double gather_ms;                              /* devices[0]: transport + assembly, events */
  double wall_ms;
} grt_gbuffer_multi_report;

int grt_gbuffer_trace_multi(grt_scene* scene, int n_devices, const int* devices, uint32_t band_rows,
                            grt_gbuffer** out, grt_stats* stats, grt_gbuffer_multi_report* report);

/* Host only.  The shape key of a scene descriptor. */
void grt_gbuffer_shape_of(const grt_scene_desc* desc, grt_gbuffer_shape* out);
/* 0 when a g-buffer traced under `traced` can be shaded under `appearance` (equal shape
 * keys), else -EINVAL and grt_last_error() names the first differing field. */
int grt_gbuffer_compatible(const grt_scene_desc* traced, const grt_scene_desc* appearance);
/* The same for a buffer's recorded key. */
int grt_gbuffer_shape_compatible(const grt_gbuffer_shape* traced, const grt_scene_desc* appearance);

/* Host only: the g-buffer file.  Little-endian, no padding:
 *   8 B   magic "GRTGBUF\0"
 *   u32   version (GRT_GBUFFER_FILE_VERSION), u32 sizeof(grt_gbuffer_info)
 *   grt_gbuffer_info
 *   layer_start u64[n_pixels + 1]; sky_u, sky_v, sky_redshift f64[n_pixels];
 *   u, v, redshift, radius f64[n_layers]; steps u32[n_pixels];
 *   status, stop u8[n_pixels]; object u8[n_layers]
 * Reading takes two calls: with arrays == NULL it checks the header and the file length
 * and fills *info (the sizes); with the arrays allocated it fills them.  It rejects, with
 * -EINVAL and a message, a wrong magic or version, sizes that disagree with each other or
 * with the file length, a layer_start that is not non-decreasing from 0 to n_layers, and an
 * object index >= shape.n_objects; -EIO when the file cannot be read or written. */
#define GRT_GBUFFER_FILE_VERSION 1
int grt_gbuffer_write_file(const char* path, const grt_gbuffer_info* info, const grt_gbuffer_arrays* arrays);
int grt_gbuffer_read_file(const char* path, grt_gbuffer_info* info, const grt_gbuffer_arrays* arrays);

/* ---- Supersampled g-buffer: the adaptive frame, re-shaded bit for bit ----
 * A buffer optionally holds a sub-sample set: for some of its pixels, the samples_per_axis^2
 * jittered sub-rays of the adaptive pass (raytracer.rs:320-384), each reduced to exactly
 * what a 1-spp ray is reduced to above.  The jitter of a sub-ray depends on (row, col,
 * stratum, samples_per_axis) alone, so a held pixel's sub-rays serve every appearance; which
 * pixels an adaptive frame supersamples depends on the appearance, so the set grows.
 *   sub_pixel[n_sub_pixels]   pixel index in the buffer's rectangle, in append order (block b);
 *   a second grt_gbuffer_arrays over n_sub_rays = n_sub_pixels * spa^2 rays and n_sub_layers
 *   layers: sub-ray b * spa^2 + s is stratum s (row-major, spa columns) of block b.
 * The set is append-only; it never holds a GRT_FLAG_HIT_OVERFLOW ray.  Still outside the
 * buffer: row shards, the multi-GPU frame, VolumetricDisc scenes, the fused arithmetic.  A
 * camera sequence's buffers (grt_gbuffer_trace_sequence) start without a set; each takes one
 * as any buffer does, per frame, with a tracer that has the frame's camera, or all of them
 * in stacked traces (grt_gbuffer_supersample_sequence). */
typedef struct grt_gbuffer_sub_info {
  uint32_t samples_per_axis; /* 0: the buffer holds no set */
  uint32_t _pad;
  uint64_t n_sub_pixels;
  uint64_t n_sub_rays;       /* n_sub_pixels * samples_per_axis^2 */
  uint64_t n_sub_layers;
} grt_gbuffer_sub_info;

typedef struct grt_gbuffer_section_report {
  uint64_t n_selected; /* pixels the selection picked under this appearance */
  uint64_t n_held;     /* of those, held by the set when the call began */
  uint64_t n_traced;   /* of those, traced and appended by this call */
  uint64_t n_missing;  /* of those, still missing when the call returned (-ENODATA) */
  double shade_ms;     /* event time: 1-spp shade, floor, select, split, sub-ray shade, average */
  double trace_ms;     /* event time of the top-up's traces, scan and fill */
  grt_stats top_up;    /* the top-up's counters (rays = n_traced * spa^2) */
} grt_gbuffer_section_report;

/* Trace the sub-rays of `pixels` (n indices into the buffer's rectangle, any order,
 * duplicates allowed) under `tracer` and append them to the set.  Pixels already held are
 * skipped; the rest are appended in ascending pixel index, traced with the exact kernels
 * in chunks of grt_set_sub_chunk sub-rays.  A chunk that loses hit candidates grows the pool
 * and is traced again (at most 3 traces, else -ENOMEM).  -EINVAL when spa is 0 or differs
 * from the set's, when a pixel is outside the rectangle, when the tracer's shape key
 * differs from the buffer's, or when its camera, max_steps, max_radius, step_size, epsilon
 * or horizon_epsilon differ byte for byte from the recorded ones (grt_last_error names the
 * field): the sub-rays must belong to the frame the buffer holds.  stats (nullable): the
 * counters of this call's traces. */
int grt_gbuffer_supersample(grt_scene* tracer, grt_gbuffer* gb, uint32_t samples_per_axis, uint64_t n,
                            const uint32_t* pixels, grt_stats* stats);
/* The adaptive frame of the buffer under `appearance`: what grt_render_section_ex writes for
 * the buffer's rectangle of a scene with this appearance and the traced geometry, camera
 * and integration parameters, bit for bit (f64 xyza, class and status of the 1-spp pass,
 * n_supersampled, the failed sub-sample list).  1-spp shade, luminance floor, selection,
 * then the held sub-rays of the selected pixels shaded and averaged, all on the buffer's
 * device.  Selected pixels the set does not hold: with `tracer` (nullable; may be
 * `appearance`) they are traced once and appended (grt_gbuffer_supersample's rules), else
 * the call returns -ENODATA with report->n_missing set and the outputs untouched.  With
 * sampling_mask_xyza the selected pixels are painted and nothing is supersampled; with
 * cfg->enabled == 0 and no mask the frame is the 1-spp one.  cfg->samples_per_axis must
 * equal the set's when one exists.  class_out, status_out, n_supersampled, failures and
 * report are nullable. */
int grt_gbuffer_shade_section(grt_scene* appearance, grt_gbuffer* gb, const grt_adaptive_config* cfg,
                              const double* sampling_mask_xyza, grt_scene* tracer, double* xyza_out,
                              uint8_t* class_out, uint8_t* status_out, uint64_t* n_supersampled,
                              grt_subsample_failures* failures, grt_gbuffer_section_report* report);
int grt_gbuffer_sub_info_get(const grt_gbuffer* gb, grt_gbuffer_sub_info* out);
/* Copy the set to the host: sub_pixel[n_sub_pixels] and the arrays sized by
 * grt_gbuffer_sub_info_get (n_sub_rays for the per-pixel ones, n_sub_layers per layer). */
int grt_gbuffer_sub_download(const grt_gbuffer* gb, uint32_t* sub_pixel, const grt_gbuffer_arrays* host);
/* Replace the buffer's set by host arrays.  They are held to the checks a file gets, and
 * sub_pixel must be < n_pixels and free of duplicates, the statuses free of
 * GRT_FLAG_HIT_OVERFLOW: -EINVAL, never a crash. */
int grt_gbuffer_sub_upload(grt_gbuffer* gb, const grt_gbuffer_sub_info* sub, const uint32_t* sub_pixel,
                           const grt_gbuffer_arrays* host);

/* Host only: the set's sidecar file (a .grtg file keeps its bytes and its version).
 * Little-endian, no padding:
 *   8 B   magic "GRTGSUB\0"
 *   u32   version (GRT_GBUFFER_SUB_FILE_VERSION), u32 sizeof(grt_gbuffer_info)
 *   grt_gbuffer_info          a copy of the buffer's, binding the set to it
 *   grt_gbuffer_sub_info
 *   sub_pixel u32[n_sub_pixels]
 *   the twelve arrays in the .grtg order, over n_sub_rays and n_sub_layers
 * Reading takes two calls, as grt_gbuffer_read_file: arrays == NULL checks the header and
 * the length and fills *sub.  `info` is the buffer's: a sidecar whose copy differs from it
 * (the device aside) is refused with -EINVAL, as are a wrong magic or version, sizes that
 * disagree, and arrays that fail grt_gbuffer_sub_upload's checks. */
#define GRT_GBUFFER_SUB_FILE_VERSION 1
int grt_gbuffer_sub_write_file(const char* path, const grt_gbuffer_info* info, const grt_gbuffer_sub_info* sub,
                               const uint32_t* sub_pixel, const grt_gbuffer_arrays* arrays);
int grt_gbuffer_sub_read_file(const char* path, const grt_gbuffer_info* info, grt_gbuffer_sub_info* sub,
                              uint32_t* sub_pixel, const grt_gbuffer_arrays* arrays);

/* ---- geometry buffers of a camera sequence: trace the animation once, re-shade it ----
 * K cameras over one resident scene, traced stacked as grt_render_sequence traces them (one
 * 1-spp trace of the sequence unit per launch group of grt_set_sequence_group, the group
 * arithmetic that call uses, always the exact arithmetic), each frame kept as a g-buffer. */
typedef struct grt_gbuffer_sequence_report {
  uint32_t n_frames, n_launches, frames_per_launch, n_traces; /* n_traces counts re-traces after a pool overflow */
  double wall_ms, trace_ms, fill_ms;                          /* host clock; summed event times */
} grt_gbuffer_sequence_report;

/* Trace n_cameras whole frames of `scene` on `device` and keep one g-buffer per frame.  Every
 * camera must have the scene's rows and cols, else -EINVAL (n_cameras = 0 too); -ENOTSUP for
 * a scene with a VolumetricDisc.  out[k] is an ordinary grt_gbuffer: its info holds
 * cameras[k], the rectangle (0, 0, rows, cols), the scene's shape key and integration
 * parameters, and info and arrays are byte for byte what grt_gbuffer_trace returns for a scene
 * created with that camera, so every grt_gbuffer_* call takes it.  A launch group whose trace
 * loses hit candidates grows the pool to its need and is traced again as a whole (at most 3
 * traces, else -ENOMEM): no buffer holds a GRT_FLAG_HIT_OVERFLOW ray.  On any failure every
 * buffer the call made is destroyed and out[0 .. n_cameras) is NULL.  stats (nullable): the
 * counters of all traces, kernel_ms their event time.  grt_gbuffer_trace_times of such a
 * buffer reports the times of its whole launch group (the stacked trace(s); the scan, the
 * fill and the split into frames), not a share of them.  report is nullable. */
int grt_gbuffer_trace_sequence(grt_scene* scene, int device, uint32_t n_cameras, const grt_camera_desc* cameras,
                               grt_gbuffer** out /* [n_cameras] */, grt_stats* stats,
                               grt_gbuffer_sequence_report* report);
/* Shade n buffers of equal rows x cols on one device under `appearance` in stacked launches:
 * one kernel launch and one set of device-to-host copies per group of grt_set_sequence_group
 * rays (whole buffers, at least one), not one per buffer.  out: host arrays, frame-major
 * [n][rows][cols]; xyza, xyza64, ray_class and status are written where non-null (at least
 * one of xyza and xyza64 is required); stop and steps, where non-null, are copies of the
 * buffers' recorded ones.  Frame k equals grt_gbuffer_shade(appearance, buffers[k]) bit for
 * bit.  -EINVAL for n = 0, a buffer on another device than buffers[0], another rows x cols,
 * or a shape key that differs from the appearance's (grt_last_error names the frame index
 * and the field).  kernel_ms (nullable): summed event time of the shade launches. */
int grt_gbuffer_shade_sequence(grt_scene* appearance, uint32_t n, grt_gbuffer* const* buffers,
                               const grt_frame_out* out, float* kernel_ms);
/* grt_gbuffer_supersample for n buffers at once, the traces stacked: the sub-rays of
 * pixels[k] (n_pixels[k] indices into buffers[k], any order, duplicates allowed) are traced
 * and appended to buffers[k]'s own set.  Per buffer the rules are grt_gbuffer_supersample's
 * (held pixels skipped, the rest ascending and unique); the n lists are concatenated
 * frame-major and cut into chunks of grt_set_sub_chunk sub-rays, so a chunk may span frames.
 * A chunk is one offset-list trace of the sequence unit over the stack of n * rows rows, each
 * ray with the camera its buffer recorded (info.camera) and the jitter of its frame's own
 * (row, col); one layer scan and one fill, then the cut into the sets.  A chunk that loses
 * hit candidates grows the pool and is traced again (at most 3 traces, else -ENOMEM).  Every
 * set is byte for byte (grt_gbuffer_sub_info, sub_pixel, the twelve arrays) what
 * grt_gbuffer_supersample leaves with a tracer created with that frame's camera.
 * `tracer`: its shape key and max_steps, max_radius, step_size, epsilon and horizon_epsilon
 * must equal every buffer's record byte for byte, its camera's rows and cols the buffers';
 * its camera is otherwise not used.  -EINVAL, grt_last_error naming the frame index (and the
 * field where grt_gbuffer_supersample names one): n = 0, a buffer listed twice, buffers on
 * different devices or of different rows x cols, a buffer that is not a whole frame
 * (rectangle (0, 0, camera.rows, camera.cols)), samples_per_axis 0, above 64 or different
 * from an existing set's, a pixel outside its buffer, more than INT_MAX - 1 stacked sub-rays.
 * After a failure every set is still a valid set: whole pixels only, grown by the chunks that
 * were complete.  stats (nullable): the counters of all traces.  report (nullable):
 * n_launches counts the chunks, n_traces the traces with the re-traces, frames_per_launch
 * is 0 (a chunk is cut over sub-rays, not frames). */
int grt_gbuffer_supersample_sequence(grt_scene* tracer, uint32_t n, grt_gbuffer* const* buffers,
                                     uint32_t samples_per_axis, const uint64_t* n_pixels /* [n] */,
                                     const uint32_t* const* pixels /* [n] */, grt_stats* stats,
                                     grt_gbuffer_sequence_report* report);

typedef struct grt_gbuffer_section_sequence_report {
  uint32_t n_frames, n_launches;                    /* n_launches: launch groups of the shade */
  uint64_t n_selected, n_held, n_traced, n_missing; /* grt_gbuffer_section_report's, summed over the frames */
  double wall_ms, shade_ms, trace_ms;               /* host clock; summed event times, as grt_gbuffer_section_report */
  grt_stats top_up;                                 /* the stacked top-up's counters */
} grt_gbuffer_section_sequence_report;

/* grt_gbuffer_shade_section for n whole-frame buffers of one size on one device, stacked:
 * frame k of the outputs is what grt_gbuffer_shade_section(appearance, buffers[k], cfg, mask,
 * tracer_k, ...) writes, bit for bit (xyza64, ray_class, status, n_supersampled[k],
 * failures[k]), tracer_k being a scene with the frame's camera; hence grt_render_section_ex
 * of the appearance with camera k.  out: host arrays, frame-major [n][rows][cols]; xyza64 is
 * required, ray_class and status are written where non-null, stop and steps are copies of
 * the recorded ones (as grt_gbuffer_shade_sequence), xyza is not written.
 * Per launch group (whole buffers, grt_set_sequence_group rays), on one stream without a
 * host round trip: one stacked 1-spp shade; per frame, on its slice, the luminance floor,
 * the selection and its compaction (neither sees another frame); with the mask the paint;
 * else one split of all the selections into held and missing, each pixel looked up in its
 * own buffer's set, then per chunk of grt_set_sub_chunk sub-rays one stacked sub-ray shade
 * and the average; one copy of the counters and one set of device-to-host copies.
 * Selected pixels that the sets do not hold: without `tracer`, -ENODATA, per_frame and
 * report->n_missing filled, the frame outputs untouched and no set changed; with `tracer`
 * (may be `appearance`; grt_gbuffer_supersample_sequence's rules) all frames' missing pixels
 * are traced in one stacked top-up and the groups that missed some are shaded again.
 * -EINVAL: grt_gbuffer_supersample_sequence's refusals (the samples_per_axis and tracer ones
 * only where sub-rays are shaded), no out->xyza64, a shape key that differs from the
 * appearance's (frame index and field named).  With cfg->enabled == 0 and no mask the frames
 * are the 1-spp ones.  failures[k].count is exact; the list holds the frame's first
 * `capacity` records in (pixel, stratum) order of those the device kept.  per_frame
 * (nullable) [n][4]: selected, held when the call began, traced by it, still missing.
 * n_supersampled, failures, per_frame and report are nullable. */
int grt_gbuffer_shade_section_sequence(grt_scene* appearance, uint32_t n, grt_gbuffer* const* buffers,
                                       const grt_adaptive_config* cfg, const double* sampling_mask_xyza,
                                       grt_scene* tracer /* nullable */, const grt_frame_out* out,
                                       uint64_t* n_supersampled /* [n] */, grt_subsample_failures* failures /* [n] */,
                                       uint64_t* per_frame /* [n][4] */, grt_gbuffer_section_sequence_report* report);

/* ---- the disc's orbital motion from one geometry buffer ----
 * The shade pass takes a disc emitter's four-velocity from a circular orbit with
 *   Omega(r) = sqrt(M) / (r^1.5 + a sqrt(M)),  M = radius / 2
 * (the Doppler shift and the beaming come from it), so a disc whose texture orbits at that
 * rate is the animation of the very scene being rendered.  It needs no geodesic: a buffer
 * keeps, per layer, the disc's texture coordinates and its radius.  The rule:
 *   orbit_rate(geometry, r_s, a, r): +0.0 for GRT_GEOM_EUCLIDEAN and
 *     GRT_GEOM_EUCLIDEAN_SPHERICAL (the emitter is at rest there); else m = 0.5 r_s,
 *     sm = sqrt(m), sm / (pow(r, 1.5) + a sm);
 *   orbit_uv(omega, t, u, v): th = omega t; (u, v) unchanged bit for bit when th == 0 or th is
 *     not finite; else (s, c) = sincos(th), du = u - 0.5, dv = v - 0.5,
 *     u' = 0.5 + (du c + dv s), v' = 0.5 + (dv c - du s)
 * -- matter seen at in-plane angle phi at time t sat at phi - Omega t at time 0, and a disc's
 * uv is 0.5 + 0.5 rho (cos phi, sin phi), so the lookup point turns about (0.5, 0.5).  It
 * applies to the layers of GRT_OBJ_DISC objects with r = the layer's recorded radius; sphere
 * layers and the celestial sphere are static.  r_s and a are the appearance scene's (the
 * shape key makes them the traced ones).
 * "Fast light": all layers of a frame are shaded at the same coordinate time t, and light-travel
 * delay is ignored ("Retarded time" below adds it for buffers traced with their lapse).
 * Host and device state the rule with the same operations in the same order, without
 * contraction, over the same glibc-exact pow and sincos: they agree bit for bit for
 * |Omega t| < 105414350 (the range of the exact sincos); beyond it the device uses the
 * fallback the render uses, within 1 ulp.
 * Not covered: VolumetricDisc scenes (refused as everywhere), the fused
 * arithmetic, stacked adaptive frames over many times (loop grt_gbuffer_shade_section_at),
 * times combined with camera sequences, the multi-GPU frame, user-given rotation laws. */
/* d(phi)/dt of the shade pass's disc emitter at radius r; +0.0 for the flat charts.
 * -EINVAL: unknown geometry, null out. */
int grt_orbit_rate(int32_t geometry, double radius, double a, double r, double* omega);
/* Host restatement of the rule over layer arrays (a buffer's or a sub-sample set's): the
 * reference the device is tested against, and a tool for users who post-process downloaded
 * arrays.  -EINVAL: null pointer, non-finite time, unknown geometry, an object index >=
 * shape->n_objects (nothing is written then).  u_out / v_out may alias u / v. */
int grt_gbuffer_orbit_uv(const grt_gbuffer_shape* shape, uint64_t n_layers, const uint8_t* object,
                         const double* u, const double* v, const double* radius, double time,
                         double* u_out, double* v_out);
/* n_times frames of one buffer under `appearance`, frame k at times[k], frame-major in `out`
 * (fields as grt_gbuffer_shade_sequence; stop and steps are copies of the recorded ones per
 * frame): one kernel launch and one set of device-to-host copies per group of
 * grt_set_sequence_group rays (whole frames, at least one).  Frame k equals grt_gbuffer_shade
 * of the buffer whose disc layers' (u, v) went through grt_gbuffer_orbit_uv at times[k], bit
 * for bit; a time of 0 gives grt_gbuffer_shade's frame.  -EINVAL for n_times = 0, a
 * non-finite time, a shape key that differs (grt_last_error names the field), or neither
 * xyza nor xyza64 given.  kernel_ms (nullable): summed event time of the launches. */
int grt_gbuffer_shade_times(grt_scene* appearance, const grt_gbuffer* gb, uint32_t n_times,
                            const double* times, const grt_frame_out* out, float* kernel_ms);
/* grt_gbuffer_shade_section at one time: the same pipeline with the 1-spp pass and the
 * sub-ray pass shaded at `time`.  The sub-sample set stays pure geometry: a top-up appends
 * the unrotated numbers grt_gbuffer_supersample leaves, and the time enters only at the
 * texture lookup.  The selection at `time` may need pixels the set lacks: the tracer /
 * -ENODATA rules are grt_gbuffer_shade_section's.  -EINVAL for a non-finite time. */
int grt_gbuffer_shade_section_at(grt_scene* appearance, grt_gbuffer* gb, const grt_adaptive_config* cfg,
                                 const double* sampling_mask_xyza, grt_scene* tracer, double* xyza_out,
                                 uint8_t* class_out, uint8_t* status_out, uint64_t* n_supersampled,
                                 grt_subsample_failures* failures, grt_gbuffer_section_report* report,
                                 double time);

/* Retarded time: each layer's light-travel time, and the orbital motion shaded with it.
 *
 * The integrator carries the chart's coordinate time as y[0].  A lapse trace keeps, per
 * layer, lapse = (y[0] lerped over the hit's window by the chord parameter) - (the camera's
 * y[0]): the coordinate time the light of that layer took to the camera, negated, since
 * the traced momenta are past-directed -- every lapse is <= 0.  With it the orbital motion
 * is shaded at the emission time: a disc layer is looked up at time + lapse instead of time
 * (orbit_uv(omega, time + lapse[k], u, v): one add, then the rule above), so the far side
 * of the disc and the higher-order images show the matter where it was when the light left.
 * The lapse is an optional part of a buffer, beside its twelve arrays: grt_gbuffer_arrays,
 * the .grtg format and the ABI version are as they were.  The time is the chart's own:
 * Kerr-Schild's t and Boyer-Lindquist's t differ by a function of r, so each chart's movie
 * is consistent in its own slicing and the two differ by a radius-dependent phase at time 0,
 * as their phi already do.
 * The sub-sample set takes lapses too ("Retarded time, adaptive" below).
 * Not covered: camera sequences, the multi-GPU buffer, the fused arithmetic, VolumetricDisc
 * scenes, and a time along the ray for the celestial sphere, which is static. */
/* grt_gbuffer_trace through the kernels that record hit times: the same info and twelve
 * arrays, byte for byte, the same pool-growth retries, always the exact kernels, -ENOTSUP
 * for VolumetricDisc scenes; the buffer holds its lapse (n_layers doubles). */
int grt_gbuffer_trace_lapse(grt_scene* scene, int device, uint32_t row0, uint32_t col0, uint32_t rows,
                            uint32_t cols, grt_gbuffer** out, grt_stats* stats);
/* The buffer's lapse to out[n_layers].  -ENODATA: the buffer holds none. */
int grt_gbuffer_lapse_download(const grt_gbuffer* gb, double* out);
/* Give the buffer a lapse (it replaces a held one).  -EINVAL: n_layers is not the buffer's,
 * or an entry is not finite; the buffer is unchanged then. */
int grt_gbuffer_lapse_upload(grt_gbuffer* gb, const double* lapse, uint64_t n_layers);
/* The lapse's sidecar file, by convention <buffer file>.lapse: an 8-byte magic, the u32
 * version and the u32 size of the info block, the buffer's grt_gbuffer_info (device zeroed;
 * a reader refuses a sidecar whose copy differs from `info`), a u64 n_layers, the doubles.
 * read: lapse NULL checks the file only; else lapse[info->n_layers].  -EINVAL: null
 * argument, a count other than info->n_layers, a non-finite entry, a truncated file or one
 * whose length disagrees with its sizes; -EIO: the file cannot be opened, read or written. */
#define GRT_GBUFFER_LAPSE_FILE_VERSION 1
int grt_gbuffer_lapse_write_file(const char* path, const grt_gbuffer_info* info, const double* lapse,
                                 uint64_t n_layers);
int grt_gbuffer_lapse_read_file(const char* path, const grt_gbuffer_info* info, double* lapse);
/* grt_gbuffer_orbit_uv with each disc layer at time + lapse[k].  -EINVAL as
 * grt_gbuffer_orbit_uv, and for a null or non-finite lapse (nothing is written then).
 * u_out / v_out may alias u / v. */
int grt_gbuffer_orbit_uv_retarded(const grt_gbuffer_shape* shape, uint64_t n_layers, const uint8_t* object,
                                  const double* u, const double* v, const double* radius, const double* lapse,
                                  double time, double* u_out, double* v_out);
/* grt_gbuffer_shade_times with the retarded rule: arguments, launch groups and refusals are
 * its own, plus -ENODATA for a buffer without a lapse.  Frame k equals grt_gbuffer_shade of
 * the buffer whose disc layers' (u, v) went through grt_gbuffer_orbit_uv_retarded at
 * times[k], bit for bit, in the range grt_gbuffer_shade_times promises it. */
int grt_gbuffer_shade_times_retarded(grt_scene* appearance, const grt_gbuffer* gb, uint32_t n_times,
                                     const double* times, const grt_frame_out* out, float* kernel_ms);

/* Retarded time, adaptive: lapses for the sub-sample set, and the adaptive frame shaded with them.
 *
 * A set is timed or untimed.  A timed set holds one lapse per sub-layer (n_sub_layers doubles,
 * indexed as the set's layer arrays are), beside its twelve arrays: grt_gbuffer_sub_info, the
 * .sub format and the ABI version are as they were.  The kind is fixed when the first block is
 * appended: grt_gbuffer_supersample_lapse and a top-up of grt_gbuffer_shade_section_at_retarded
 * make an empty set timed, the other entries make it untimed, and every later fill of a set
 * keeps its kind whichever entry asked for it (a timed set is always filled through the kernels
 * that record hit times; the twelve arrays are byte for byte the same either way).
 * grt_gbuffer_sub_upload leaves an untimed set, grt_gbuffer_sub_lapse_upload makes it timed,
 * grt_gbuffer_sub_clear drops a set of either kind.  The stacked calls
 * (grt_gbuffer_supersample_sequence, grt_gbuffer_shade_section_sequence) trace with camera
 * tables, which the lapse kernels do not take: they return -EINVAL, naming the frame, for a
 * buffer whose set is timed.
 * Not covered: several times in one stacked adaptive call (loop
 * grt_gbuffer_shade_section_at_retarded), one top-up for a whole movie, camera sequences, the
 * multi-GPU buffer, the fused arithmetic, VolumetricDisc scenes. */
/* grt_gbuffer_supersample into a timed set: its arguments, rules and refusals, the sub-rays
 * traced through the kernels that record hit times.  -EINVAL when the set holds blocks and is
 * untimed (grt_last_error gives its pixel count). */
int grt_gbuffer_supersample_lapse(grt_scene* tracer, grt_gbuffer* gb, uint32_t samples_per_axis, uint64_t n,
                                  const uint32_t* pixels, grt_stats* stats);
/* 1: the buffer's set is timed; 0: untimed, or no set; -EINVAL: null buffer. */
int grt_gbuffer_sub_has_lapse(const grt_gbuffer* gb);
/* Drop the buffer's set: its arrays, its pixel map and its kind.  The buffer then holds no set. */
int grt_gbuffer_sub_clear(grt_gbuffer* gb);
/* The set's lapse to out[n_sub_layers].  -ENODATA: the set is untimed, or there is none. */
int grt_gbuffer_sub_lapse_download(const grt_gbuffer* gb, double* out);
/* Give the set a lapse (it replaces a held one) and so make it timed.  -EINVAL: the buffer
 * holds no set, n is not the set's n_sub_layers, or an entry is not finite; nothing changes then. */
int grt_gbuffer_sub_lapse_upload(grt_gbuffer* gb, const double* lapse, uint64_t n);
/* grt_gbuffer_shade_section_at under the retarded rule: the same arguments and pipeline, the
 * 1-spp pass with the buffer's lapse and the sub-ray pass with the set's, each disc layer at
 * time + its lapse.  The frame equals grt_gbuffer_shade_section of the buffer whose arrays and
 * set arrays went through grt_gbuffer_orbit_uv_retarded at `time`, bit for bit.  -ENODATA: the
 * buffer holds no lapse; the sub-ray pass would run on a set that holds blocks and is untimed
 * (grt_last_error gives its pixel and layer counts); or, as ever, pixels are missing and there
 * is no tracer.  A top-up fills an empty set timed.  With a mask or cfg->enabled == 0 the set
 * is not touched and only the buffer's lapse is needed. */
int grt_gbuffer_shade_section_at_retarded(grt_scene* appearance, grt_gbuffer* gb, const grt_adaptive_config* cfg,
                                          const double* sampling_mask_xyza, grt_scene* tracer, double* xyza_out,
                                          uint8_t* class_out, uint8_t* status_out, uint64_t* n_supersampled,
                                          grt_subsample_failures* failures, grt_gbuffer_section_report* report,
                                          double time);
/* The set's lapse sidecar, by convention <buffer file>.sub.lapse.  Little-endian, no padding:
 *   8 B   magic "GRTGSLP\0"
 *   u32   version (GRT_GBUFFER_SUB_LAPSE_FILE_VERSION), u32 sizeof(grt_gbuffer_info)
 *   grt_gbuffer_info          the buffer's, device zeroed
 *   grt_gbuffer_sub_info      the set's: a .sub that grew since leaves this sidecar stale
 *   f64[n_sub_layers]
 * read: lapse NULL checks the file only; else lapse[sub->n_sub_layers], written only after
 * every check.  `info` and `sub` are the buffer's and the set's.  -EINVAL: null argument, an
 * info or sub-info that differs from the file's, a count other than sub->n_sub_layers, a
 * non-finite entry, a wrong magic or version, a truncated file or one whose length disagrees
 * with its sizes; -EIO: the file cannot be opened, read or written. */
#define GRT_GBUFFER_SUB_LAPSE_FILE_VERSION 1
int grt_gbuffer_sub_lapse_write_file(const char* path, const grt_gbuffer_info* info, const grt_gbuffer_sub_info* sub,
                                     const double* lapse, uint64_t n_sub_layers);
int grt_gbuffer_sub_lapse_read_file(const char* path, const grt_gbuffer_info* info, const grt_gbuffer_sub_info* sub,
                                    double* lapse);

/* The device hit pool that keeps the window candidates past a ray's GRT_MAX_HITS slots
 * (no reference counterpart: the reference's per-ray Vec grows, scene.rs:139-152).
 * A trace starts with the pool at its minimum (grt_set_hit_pool_min, 2^20 records) or
 * the size a measured need grew it to; a trace that needs more flags the pixels it could
 * not keep (GRT_FLAG_HIT_OVERFLOW, grt_stats.hit_overflows).  The synchronous calls then
 * trace those pixels again (growing the pool to their need).  After an *_async call whose
 * d_stats[3] is non-zero, call this with records = 0 (waits for the device, then sizes
 * the pool for the largest trace since the last call) or with an explicit record count,
 * and trace again.  *capacity (nullable) returns the pool size in records. */
int grt_hit_pool_reserve(grt_scene* scene, int device, uint64_t records, uint64_t* capacity);
/* Smallest pool a trace allocates (default 2^20 records; tests lower it to exercise a
 * full pool).  Applies to pools allocated or grown afterwards. */
int grt_set_hit_pool_min(uint64_t records);
/* Sub-rays per supersample trace launch (default 0 = 2^21; at least one pixel's spa^2
 * sub-rays per launch).  The supersample pass runs the selected pixels in chunks of
 * this many sub-rays, each chunk's live count read on the device.  Scheduling only:
 * results are identical for every chunk size (tests force several partly filled ones). */
int grt_set_sub_chunk(uint64_t sub_rays);

/* ---- adaptive supersampling of a frame split across GPUs -------
 * render_section_to_cie_buffer_supersampled (raytracer.rs:257-318) with the frame's
 * rows spread over processes.  Per rank:
 *   1. grt_render_shard_async(..., d_xyza64, ...): the 1-spp pass of its row bands;
 *   2. allgather of every pixel's (Y, alpha) and class, frame order (17 B per pixel:
 *      the selection stencil reads its 8 neighbours, which may belong to other ranks,
 *      and the luminance floor is a percentile over the whole frame);
 *   3. grt_adaptive_min_luminance over the frame's Y: identical on every rank;
 *   4. grt_supersample_shard: selection of the shard's pixels, samples_per_axis^2
 *      jittered rays per selected pixel, ordered average into the shard's f64 XYZA.
 * The result is identical to grt_render_section over the whole frame. */

/* resolve_minimum_luminance (raytracer.rs:118-129): cfg->minimum_luminance when set,
 * else 1e-3 x the ((n-1) * 0.99)-th luminance in f64::total_cmp order (0 when n = 0). */
double grt_adaptive_min_luminance(const double* lum, uint64_t n, const grt_adaptive_config* cfg);
/* The same value from n DEVICE luminances d_y[stride * i] on `device`, selected on the
 * GPU (radix sort in total_cmp order; synchronises `stream`).  Returns 0 or -errno. */
int grt_adaptive_min_luminance_device(int device, void* stream, const double* d_y, uint32_t stride, uint64_t n,
                                      const grt_adaptive_config* cfg, double* out);

/* collect_pixels_to_supersample (raytracer.rs:386-458) over the local pixels of shard
 * `sh` + supersample (:320-384), on `device`, enqueued on `stream` and synchronised
 * before returning (the selection count sizes the second trace).
 * d_frame_ya: (Y, alpha) per frame pixel, 2 f64, frame order; d_frame_class: RayClass
 * per frame pixel; d_xyza64: the shard's 1-spp f64 XYZA (local rows, grt_render_shard
 * order), overwritten in place for the selected pixels; sampling_mask_xyza (host,
 * 4 f64, nullable): paint the selected pixels instead (--show-sampling-mask,
 * raytracer.rs:285-295).  d_stats: 4 uint64 device counters, accumulated. */
int grt_supersample_shard(grt_scene* scene, int device, void* stream, const grt_row_shard* sh,
                          const grt_adaptive_config* cfg, double min_lum, const double* d_frame_ya,
                          const uint8_t* d_frame_class, const double* sampling_mask_xyza,
                          double* d_xyza64, uint64_t* n_supersampled, uint64_t* d_stats);
/* The same, asynchronous on `stream` with everything on the device: the floor is
 * *d_min_lum when d_min_lum is non-null (grt_adaptive_floor_device), else min_lum; the
 * selection count goes to *d_n_supersampled (device uint64, nullable).  failures
 * (nullable) synchronises `stream` to return the failed sub-samples (frame pixel
 * indices). */
int grt_supersample_shard_device(grt_scene* scene, int device, void* stream, const grt_row_shard* sh,
                                 const grt_adaptive_config* cfg, double min_lum, const double* d_min_lum,
                                 const double* d_frame_ya, const uint8_t* d_frame_class,
                                 const double* sampling_mask_xyza, double* d_xyza64,
                                 uint64_t* d_n_supersampled, uint64_t* d_stats,
                                 grt_subsample_failures* failures);
/* resolve_minimum_luminance's relative floor of n DEVICE luminances d_y[stride * i],
 * written to *d_min_lum (device double) on `stream` without a host copy (n <= INT_MAX;
 * n = 0 gives +0.0).  A configured minimum_luminance is the caller's constant instead. */
int grt_adaptive_floor_device(grt_scene* scene, int device, void* stream, const double* d_y, uint32_t stride,
                              uint64_t n, double* d_min_lum);

/* The image files of Raytracer::render_section (raytracer.rs:460-497): an 8-bit RGB
 * PNG, and the Radiance .hdr that stores XYZ as its RGB channels (f32, RGBE). */
int grt_write_png_rgb(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height);
int grt_write_hdr_xyz(const char* path, const double* xyza, uint32_t width, uint32_t height);

/* ---- whole trajectories (render-ray / render-ray-at) ------ */
/* Integrator::integrate keeping every Step (integrator.rs:78-174), as
 * Raytracer::integrate_ray_at_point (raytracer.rs:499-507, `render-ray`) and
 * integrate_and_save_ray (cli/shared.rs:107-129, `render-ray-at`) use it.  Ray k's
 * records are steps_out[(k * capacity + i) * 9 + f], i = 0 .. min(n_steps[k], capacity)
 * - 1, f = 0: affine parameter t; 1..4: position x^mu in the geometry's own chart;
 * 5..8: momentum_from_state p^mu.  Record 0 is the initial state.  n_steps[k] counts
 * every step, also those beyond `capacity`; stop_out is a grt_stop_reason, status_out a
 * grt_status (GRT_ERR_MAX_STEPS_REACHED: rkf45's Err, the reference writes no CSV). */
int grt_trace_pixels(grt_scene* scene, int device, uint64_t n, const double* rows,
                     const double* cols, uint64_t capacity, double* steps_out,
                     uint64_t* n_steps, uint8_t* stop_out, uint8_t* status_out);
/* Rays given by position and contravariant momentum in the geometry's chart (n x 4). */
int grt_trace_rays(grt_scene* scene, int device, uint64_t n, const double* positions,
                   const double* momenta, uint64_t capacity, double* steps_out,
                   uint64_t* n_steps, uint8_t* stop_out, uint8_t* status_out);

/* ---- invariant monitors (off the render path) --------------------------------- */
/* The reference's per-ray health checks over a rows x cols rectangle, re-integrating
 * each ray with the monitors on:
 *  - the null condition of the camera ray: Scene::color_of_ray logs an error when
 *    |k.k| >= 1e-10 (scene.rs:116-124);
 *  - the debug-build drift monitors of Integrator::integrate (integrator.rs:91-146): the
 *    largest |k.k| over the accepted steps and the largest drift of each constant of
 *    motion (get_constants_of_motion: E, L_z, and Carter's Q for KerrBL) from its value at
 *    step 0, relative when |initial| > 1e-12, warned above 1e-4 (report_drifts, :176-201).
 *    Rays whose rkf45 fails return Err before report_drifts and report no drift. */
typedef struct grt_health {
  uint64_t rays;
  uint64_t failed;                 /* rkf45 Err (MaxStepsReached): no drift report          */
  uint64_t null_violations;        /* camera rays with |k.k| >= 1e-10                        */
  double max_null;                 /* largest |k.k| of a camera ray                         */
  uint64_t kk_drift_rays;          /* rays whose largest |k.k| along the path > 1e-4         */
  double max_kk_drift;
  uint32_t n_constants;            /* 2 (E, L_z) or 3 (KerrBL: E, L_z, Q)                    */
  uint32_t _pad;
  uint64_t constant_drift_rays[3]; /* rays whose drift of constant c > 1e-4                  */
  double max_constant_drift[3];
} grt_health;
/* per_ray (nullable): rows*cols x 5 doubles -- |k.k| of the camera ray, largest |k.k| along
 * the path, largest drift of E, L_z, Q (0 where not defined). */
int grt_health_pixels(grt_scene* scene, int device, uint32_t row0, uint32_t col0, uint32_t rows,
                      uint32_t cols, grt_health* out, double* per_ray);

/* render_ray_at's initial ray (cli/{euclidean,schwarzschild,kerr,kerr_bl}.rs): the unit
 * spatial `direction` in the local tetrad at the Cartesian `position` (t = 0), as a
 * native-chart position and contravariant momentum for grt_trace_rays.  -EINVAL when
 * the direction is degenerate or the momentum is not future-directed
 * (assert_future_directed, cli/shared.rs:79-86). */
int grt_ray_at(int32_t geometry, double radius, double a, const double position[3],
               const double direction[3], double position_out[4], double momentum_out[4]);
/* IntegratedRay::save (ray.rs:35-54): "i,t,tau,x,y,z" then one line per record
 * (step, t, Cartesian x^0..x^3), f64 printed like Rust's Display. */
int grt_write_trajectory_csv(const char* path, int32_t geometry, double a, const double* steps,
                             uint64_t n_records);
/* Rust Display of one f64 into buf (NUL-terminated, truncated to cap); returns its length. */
size_t grt_format_f64(double v, char* buf, size_t cap);

/* ---- device output stage ------------------------------- */
/* Replaces xyz_to_linear_srgb_buffer + linear_srgb_to_srgb_buffer (color.rs:204-298),
 * called by Raytracer::render_section for non-HDR files (raytracer.rs:460-497).
 * GlobalLinear needs the per-channel maxima of (linear sRGB * exposure) over the WHOLE
 * frame, folded from 0.0 (color.rs:238-258): grt_linear_max_async writes them to
 * d_max3 (3 doubles, device); a frame split across GPUs allreduces them (MAX) before
 * grt_tonemap_async.  Byte-identical to the reference (glibc pow restated on device).
 * d_xyza: n x 4 f64 (the render's xyza64 output); d_rgb: n x 3 u8.  Async on `stream`. */
int grt_linear_max_async(int device, void* stream, const double* d_xyza, uint64_t n,
                         double exposure, double* d_max3);
int grt_tonemap_async(int device, void* stream, const double* d_xyza, uint64_t n,
                      int32_t tone_mapping, double exposure, const double* d_max3,
                      uint8_t* d_rgb);
/* Host buffers in and out, same result as grt_xyz_to_srgb8, computed on `device`. */
int grt_xyz_to_srgb8_device(int device, const double* xyza, size_t n, int32_t tone_mapping,
                            double exposure, uint8_t* rgb_out);

/* Floating-point contraction of the trace (no reference counterpart: the reference's Rust
 * never fuses a*b + c).  0 = exact (default): every multiply and add rounded separately in
 * the reference's order, so pixels are bit-identical to the reference's wherever the libm
 * calls are.  1 = fused: the light charts (Euclidean, Schwarzschild,
 * KerrBL, EuclideanSpherical) run kernels compiled with FMA contraction -- the same
 * algorithm and operation order, one rounding per fused pair -- which is faster (C2 -17%,
 * C3 -13%) and keeps every robust pixel within the north-star 1e-4 relative per channel
 * (tests/test_fused.py), but no longer bit-identical; Kerr-Schild always runs exact (its
 * finite-difference metric turns the changed roundings into other step sequences), and so
 * does every scene with a GRT_OBJ_VOLUMETRIC_DISC: the gas's noise turns the last bits of a
 * window's chord into colour differences above 1e-4 on pixels that no libm probe moves
 * (DESIGN.md section 19), so such a frame is the exact frame, bit for bit, in either mode.
 * It applies to frame traces (grt_render_*, grt_supersample_shard*, grt_render_frame_multi);
 * trajectories (grt_trace_*), monitors, the work-order probe and camera sequences
 * (grt_render_sequence) always run exact.
 * Process-wide; each trace reads it once when it is enqueued. */
int grt_set_arithmetic(int mode);
int grt_get_arithmetic(void);

/* Kernel launch geometry knobs (persistent grid). 0 = library default: 256 threads per
 * block, 2w blocks per CU for an integrate kernel that keeps w waves per SIMD resident
 * (w = 3 for Schwarzschild, KerrBL and the flat charts; 2 for Kerr-Schild and scenes with
 * a VolumetricDisc).  Scheduling only: results are identical for every shape. */
int grt_set_launch_config(int blocks_per_cu, int threads_per_block);
/* Tile queue order of rectangle / shard traces: 0 = row-major 8x8 tiles; 1 = a probe
 * pass (one capped ray per tile) then the tiles with the longest predicted rays first;
 * -1 = automatic (default: probe order for Kerr-Schild / Schwarzschild when
 * max_steps >= 262144 over >= 1024 tiles; KerrBL's Mino-time rays are all short).
 * Scheduling only: every pixel's result is identical in all modes. */
int grt_set_schedule(int mode);
/* Schwarzschild tile queue grouped by sincos case.  In the far field a ray's theta hardly
 * moves, so the right-hand side's sincos stays in one of its cases (Taylor near the
 * equator, table elsewhere) for nearly every step, and a wave whose 64 rays agree on it
 * runs a straight-line form.  A small predictor kernel finds each tile's case from the
 * asymptotic direction of its corner rays, and the impact-parameter order (above) takes it
 * as the minor part of its sort key.  -1 = automatic (default: wherever the
 * impact-parameter order applies); 0 = off; 1 = forced for any Schwarzschild rectangle of
 * more than one tile, whatever grt_set_schedule says (probe-ordered traces excepted);
 * 2 = the same as 1 (it selected a pixel-level regrouping of the tiles that straddle a
 * border, which was measured, did not pay for itself and is not built).
 * Scheduling only: every pixel's result is identical in all modes. */
int grt_set_class_order(int mode);
int grt_get_class_order(void);
/* Probe-ordered traces (above) hand the queue out from both ends: on every SIMD the wave
 * in an even hardware slot takes the tiles with the longest predicted rays, at raised
 * issue priority, the others take the shortest (1 = default); 0 = one end, longest
 * first, for every wave.  Scheduling only: results are identical in both modes. */
int grt_set_two_ended(int on);
/* Long-ray hand-off of Kerr-Schild traces: once the tile queue is drained and at most
 * `threshold` rays are still integrating, they continue in a tail kernel that splits each
 * RHS evaluation over 4 lanes (one wave per SIMD).  -1 = automatic (default: on, threshold
 * = the rays the tail kernel integrates at once, 64 per CU); 0 = off; > 0 = explicit
 * threshold.  Scheduling only: every pixel's result is identical in all modes. */
int grt_set_tail(long long threshold);
/* Rays the last Kerr-Schild trace on `device` handed to the tail kernel (synchronises the
 * device; 0 before the first trace).  A diagnostic of the scheduling above. */
int grt_tail_handoffs(grt_scene* scene, int device, uint64_t* handed_off);
/* The same plus the last trace's timeline in seconds since the integrate kernel started
 * (queue drained, first hand-off, tail kernel end; 0 when not reached), and for the first
 * min(handed_off, capacity) handed-off rays their output slot and the accepted steps
 * they had taken (any pointer nullable). */
int grt_tail_report(grt_scene* scene, int device, uint64_t* handed_off, double timeline_s[3], uint64_t* slot,
                    uint64_t* step, uint64_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* GRT_API_H */
