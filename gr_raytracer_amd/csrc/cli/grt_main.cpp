// grt_main.cpp — `grt`, the command line of the MI355X build, flag-compatible with
// the reference's clap CLI (src/cli/cli.rs:5-113, src/main.rs:21-178) for `render`:
//
//   grt [--width N] [--height N] [--step-size H] [--max-steps N] [--max-radius R]
//       [--epsilon E] [--camera-position x,y,z] [--phi A] [--theta A] [--psi A]
//       [--tone-mapping reinhard|global-linear] [--show-sampling-mask]
//       [--sampling-mask-color r,g,b] --config-file scene.toml
//       render [--filename out.png|out.hdr] [--from-row N] [--from-col N]
//              [--to-row N] [--to-col N]
//     | render-sequence --camera-path P [--filename-pattern frame-%04d.png] [--first-index 0]
//     | render-ray -r ROW -c COL [--filename rendered-ray.csv]
//     | render-ray-at -p x,y,z -d x,y,z [--filename rendered-ray-at.csv]
//     | gbuffer --filename a.grtg [--adaptive | --gpus N | --devices A,B,...] [--lapse]
//     | reshade --gbuffer a.grtg [--filename out.png|out.hdr] [--adaptive]
//     | gbuffer-sequence --camera-path P --filename-pattern a-%04d.grtg [--first-index 0]
//                        [--adaptive-stacked]
//     | reshade-sequence --gbuffer-pattern a-%04d.grtg --frames K [--first-index 0]
//                        [--filename-pattern frame-%04d.png] [--adaptive-stacked]
//     | reshade-orbit --gbuffer a.grtg --times T0,DT,K --filename-pattern f-%04d.png [--retarded]
//                     [--raw-out-pattern f-%04d.raw] [--first-index 0] [--adaptive]
//                     [--adaptive-retarded]
//     | blackbody -t T [-r Z]
//     | blackbody-spectrum [--min-temperature T] [--max-temperature T] [--min-redshift Z]
//                          [--max-redshift Z] [--width N] [--height N] [-f FILE]
//
// Global options go before the subcommand, subcommand options after it (clap).
// Extra (not in the reference): --device N selects the GPU, --resource-root DIR
// resolves texture paths, --raw-out FILE dumps the f64 XYZA buffer; --gpus N (GPUs
// 0..N-1) or --devices A,B,... renders the whole frame over several GPUs of this process
// (grt_render_frame_multi: cyclic row bands of --band-rows rows, default 16, one
// gather), --gpus 1 included; --transport rccl|peer|peer-staged selects how that frame's
// blocks move (grt_set_multi_transport; rccl by default; under the peer transports
// --devices may name a GPU several times, one rank per entry); --arithmetic exact|fused
// selects grt_set_arithmetic (exact, the reference's roundings, by default).
// render-sequence (not in the reference, whose animations are one process per frame):
// the frames of a camera path -- a text file, one camera per line `x,y,z,phi,theta,psi`
// -- over one load of the scene, traced in stacked launches (grt_render_sequence); frame
// k is what `render` writes for that line's --camera-position/--phi/--theta/--psi, to
// --filename-pattern (and --raw-out, a pattern too) at index --first-index + k.
// gbuffer / reshade (not in the reference): `gbuffer` traces the whole frame at 1 spp with
// the exact kernels and writes its geometry buffer (grt_gbuffer_trace, the file of
// grt_gbuffer_write_file); `reshade` loads one, shades it under the appearance of its own
// --config-file (textures, temperatures, beaming, celestial sphere, hit threshold;
// grt_gbuffer_shade) and writes the image as `render` does, tone mapping and --raw-out
// included -- what `render` of that config writes at 1 spp, without integrating.  The scene
// must have the buffer's shape key and --width / --height its frame; the camera flags
// (--camera-position, --phi, --theta, --psi) and the integration flags are ignored by
// `reshade`: the frame is the traced one.  With --adaptive on both, the config's
// [adaptive_sampling] applies: `gbuffer` also traces the sub-rays of the pixels its own
// adaptive frame supersamples and writes them to the sidecar `<file>.sub`; `reshade` loads
// the sidecar if there is one, traces the sub-rays of the pixels its appearance selects
// and the set does not hold (with the file's camera and integration parameters), writes
// what `render` of its config writes, and rewrites the sidecar when the set grew.
// `gbuffer` with --gpus / --devices (and --transport, --band-rows) traces the 1-spp frame
// over several GPUs (grt_gbuffer_trace_multi) and writes the same bytes; --adaptive with a
// device list, and a device list on `reshade` or the sequence subcommands, are usage errors:
// the sub-rays of a multi-traced buffer are `reshade --adaptive`'s top-up on one GPU.
// gbuffer-sequence / reshade-sequence (not in the reference): the two above for a camera
// path.  `gbuffer-sequence` traces the path's frames stacked over one load of the scene
// (grt_gbuffer_trace_sequence) and writes frame k to --filename-pattern at index
// --first-index + k: the bytes `gbuffer` writes for that line's camera flags.
// `reshade-sequence` loads the --frames files of --gbuffer-pattern from --first-index on,
// shades them in stacked launches under its config's appearance (grt_gbuffer_shade_sequence)
// and writes each frame, tone-mapped on its own, as `reshade` writes it.  Neither takes
// --adaptive: a sequence's files are ordinary g-buffers, and the adaptive frame of one is
// `reshade --adaptive` of that file.  The adaptive frames of the whole path are
// --adaptive-stacked on both (grt_gbuffer_shade_section_sequence): `gbuffer-sequence` then
// also traces, in one stacked top-up, the sub-rays each frame's own adaptive frame selects
// and writes every `<file>.sub`, the bytes `gbuffer --adaptive` writes for that line's
// camera; `reshade-sequence` builds one scene from its config with the files' recorded
// integration parameters (they must agree, as must the frame sizes: usage errors) as
// appearance and tracer, loads the sidecars that exist, tops the sets up in one stacked call,
// writes each frame as `render` of its config writes it (--show-sampling-mask included) and
// rewrites the sidecars that grew.
// reshade-orbit (not in the reference): the frames of one geometry buffer with the disc's
// texture orbiting at the shade pass's own emitter rate (grt_api.h, "the disc's orbital
// motion"): frame k at coordinate time T0 + k DT, K frames from one trace in stacked launches
// (grt_gbuffer_shade_times), each written as `reshade` writes its frame to --filename-pattern
// (and --raw-out-pattern) at index --first-index + k.  With --adaptive the frames are
// `reshade --adaptive`'s at those times, one after the other (grt_gbuffer_shade_section_at);
// the sidecar is loaded once and rewritten once at the end when the set grew.
// `gbuffer --lapse` also records each layer's light-travel time (grt_gbuffer_trace_lapse) and
// writes it to F.grtg.lapse; F.grtg has the bytes it has without the flag.  `reshade-orbit
// --retarded` reads that sidecar and shades every disc layer at its emission time
// (grt_gbuffer_shade_times_retarded); a missing sidecar is a usage error.
// `gbuffer --adaptive --lapse` fills a timed sub-sample set: the sub-rays of the same selection
// with their light-travel times, written to F.grtg.sub.lapse beside F.grtg.sub (each of the
// other three files has the bytes its flag writes alone).  `reshade-orbit --adaptive-retarded`
// is --adaptive under the retarded rule (grt_gbuffer_shade_section_at_retarded): it needs
// F.grtg.lapse, and F.grtg.sub.lapse wherever F.grtg.sub is there; a set it tops up stays
// timed, and both sidecars are rewritten once at the end when it grew.  `reshade --adaptive`
// and `reshade-orbit --adaptive` load F.grtg.sub.lapse when it is there and write it back
// with F.grtg.sub, so a timed set stays one.
#include <algorithm>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cctype>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "grt_api.h"

namespace grt_host {
bool png_encode_rgb(const std::string& path, const uint8_t* rgb, uint32_t w, uint32_t h, std::string& err);
bool png_encode_rgba(const std::string& path, const uint8_t* rgba, uint32_t w, uint32_t h, std::string& err);
std::string rust_display_f64(double v);
bool hdr_encode_rgb(const std::string& path, const float* rgb, uint32_t w, uint32_t h, std::string& err);
}

static int usage(const char* msg) {
  std::fprintf(stderr,
               "error: %s\nusage: grt [global options] --config-file FILE render [--filename F]\n"
               "       grt [global options] --config-file FILE render-sequence --camera-path P\n"
               "           [--filename-pattern frame-%%04d.png] [--first-index N]\n"
               "       grt [global options] --config-file FILE render-ray -r ROW -c COL [--filename F]\n"
               "       grt [global options] --config-file FILE render-ray-at -p X,Y,Z -d X,Y,Z [--filename F]\n"
               "       grt [global options] --config-file FILE gbuffer --filename F.grtg [--adaptive] [--lapse]\n"
               "           (--gpus N / --devices A,B,...: the 1-spp trace over several GPUs, the same file)\n"
               "       grt [global options] --config-file FILE reshade --gbuffer F.grtg [--filename F] [--adaptive]\n"
               "           (--adaptive: the config's [adaptive_sampling]; the sub-rays live in F.grtg.sub)\n"
               "           (reshade: --width/--height must be the buffer's frame; camera flags are ignored)\n"
               "       grt [global options] --config-file FILE gbuffer-sequence --camera-path P\n"
               "           --filename-pattern F-%%04d.grtg [--first-index N] [--adaptive-stacked]\n"
               "       grt [global options] --config-file FILE reshade-sequence --gbuffer-pattern F-%%04d.grtg\n"
               "           --frames K [--first-index N] [--filename-pattern frame-%%04d.png] [--adaptive-stacked]\n"
               "           (--adaptive-stacked: the adaptive frames of the sequence, the sub-rays in F-%%04d.grtg.sub)\n"
               "       grt [global options] --config-file FILE reshade-orbit --gbuffer F.grtg --times T0,DT,K\n"
               "           --filename-pattern F-%%04d.png [--raw-out-pattern F-%%04d.raw] [--first-index N] [--adaptive | --retarded]\n"
               "           [--adaptive-retarded]  (the adaptive frames under the retarded rule: F.grtg.lapse, F.grtg.sub.lapse)\n"
               "           (frame k: the disc's texture after orbiting for T0 + k DT; one trace, K frames)\n"
               "       grt [global options] blackbody -t T [-r Z]\n"
               "       grt [global options] blackbody-spectrum [--min-temperature T] [--max-temperature T]\n"
               "           [--min-redshift Z] [--max-redshift Z] [--width N] [--height N] [-f FILE]\n",
               msg);
  return 2;
}

// --transport's name of a grt_multi_transport.
static const char* transport_name(uint32_t t) {
  return t == GRT_TRANSPORT_PEER ? "peer" : t == GRT_TRANSPORT_PEER_STAGED ? "peer-staged" : "rccl";
}

// Debug form of the RaytracerError behind a grt_status (raytracer.rs:20-52).
static const char* error_debug_name(int status) {
  switch (status) {
    case GRT_ERR_MAX_STEPS_REACHED: return "IntegrationError(MaxStepsReached)";
    case GRT_ERR_NO_CIRCULAR_ORBIT: return "NoCircularOrbitPossible";
    case GRT_ERR_BELOW_RISCO: return "BelowRISCO";
    case GRT_ERR_NON_FINITE_RADIUS: return "NonFiniteRadius";
    default: return "Unknown";
  }
}

// clap's value parsers for the flag types of cli.rs:5-113: the whole string must be a
// number of the field's type (f64 / i64 / u32 / usize); anything else is an error.
static bool parse_f64(const std::string& v, double* out) {
  if (v.empty() || std::isspace((unsigned char)v[0])) return false;
  char* end = nullptr;
  *out = std::strtod(v.c_str(), &end);
  return *end == 0;
}
static bool parse_i64(const std::string& v, long long lo, unsigned long long hi, long long* out) {
  if (v.empty() || std::isspace((unsigned char)v[0])) return false;
  const bool neg = v[0] == '-';
  const std::string d = (v[0] == '+' || neg) ? v.substr(1) : v;
  if (d.empty() || d.find_first_not_of("0123456789") != std::string::npos || d.size() > 19) return false;
  const unsigned long long m = std::strtoull(d.c_str(), nullptr, 10);
  if (neg ? (lo >= 0 ? m != 0 : m > (unsigned long long)(-(lo + 1)) + 1) : m > hi) return false;
  *out = neg ? -(long long)(m - 1) - 1 : (long long)m;
  return true;
}

// impl FromStr for Color (color.rs:151-170): three comma-separated components, each
// trimmed and parsed as u8 (optional '+', decimal digits, at most 255).
static bool parse_rgb(const std::string& s, uint8_t out[3]) {
  int n = 0;
  size_t p = 0;
  while (true) {
    size_t q = s.find(',', p);
    std::string tok = s.substr(p, q == std::string::npos ? std::string::npos : q - p);
    size_t b = tok.find_first_not_of(" \t\n\r\f\v"), e = tok.find_last_not_of(" \t\n\r\f\v");
    if (b == std::string::npos) return false;
    tok = tok.substr(b, e - b + 1);
    if (tok[0] == '+') tok = tok.substr(1);
    if (tok.empty() || tok.size() > 3 || tok.find_first_not_of("0123456789") != std::string::npos) return false;
    int v = std::atoi(tok.c_str());
    if (v > 255 || n >= 3) return false;
    out[n++] = (uint8_t)v;
    if (q == std::string::npos) break;
    p = q + 1;
  }
  return n == 3;
}

static bool split_csv(const std::string& s, std::vector<double>& out) {
  out.clear();
  size_t p = 0;
  while (p <= s.size()) {
    size_t q = s.find(',', p);
    if (q == std::string::npos) q = s.size();
    std::string tok = s.substr(p, q - p);
    char* end = nullptr;
    double v = std::strtod(tok.c_str(), &end);
    if (tok.empty() || *end) return false;
    out.push_back(v);
    p = q + 1;
  }
  return true;
}

// scene.rs:178-183, :196-202: color_of_ray's lines for an error-free ray that ended on NaN
// coordinates or without a terminal event.  The Ray's Debug form is cut to its pixel
// (row, col); steps.len() = accepted steps + the initial step.
static void log_ray_event(unsigned row, unsigned col, int stop, uint32_t accepted) {
  const unsigned long long len = (unsigned long long)accepted + 1;
  if (stop == GRT_STOP_NAN)
    std::fprintf(stderr, "[grt] ERROR Ray hit NaN coordinates: Ray { row: %u, col: %u, .. } with %llu steps.\n", row,
                 col, len);
  else if (stop == GRT_STOP_NONE)
    std::fprintf(stderr, "[grt] ERROR Ray did not hit anything: Ray { row: %u, col: %u, .. } at Some(Step { .. }) "
                 "with %llu steps.\n", row, col, len);
}

// Rust's Debug form of an f64 ({:?}): Display's shortest digits, with ".0" on integral
// values and exponential notation outside 1e-4 <= |v| < 1e16 (core::fmt::float).
static std::string rust_debug_f64(double v) {
  if (std::isnan(v) || std::isinf(v)) return grt_host::rust_display_f64(v);
  const double a = std::fabs(v);
  if (a != 0.0 && (a < 1e-4 || a >= 1e16)) {
    char buf[64];
    auto res = std::to_chars(buf, buf + sizeof(buf), v, std::chars_format::scientific);  // shortest digits
    std::string sci(buf, res.ptr);
    const size_t e = sci.find('e');
    return sci.substr(0, e) + "e" + std::to_string(std::atoi(sci.c_str() + e + 1));
  }
  std::string d = grt_host::rust_display_f64(v);
  if (d.find('.') == std::string::npos) d += ".0";
  return d;
}

// CoordinateSystem's Debug form for the geometry (geometry/*.rs coordinate_system, point.rs:11)
static std::string coordinate_system_debug(const grt_scene_desc* d) {
  switch (d->geometry) {
    case GRT_GEOM_SCHWARZSCHILD:
    case GRT_GEOM_EUCLIDEAN_SPHERICAL: return "Spherical";
    case GRT_GEOM_KERR_BL: return "BoyerLindquist { a: " + rust_debug_f64(d->a) + " }";
    default: return "Cartesian";  // Euclidean, Kerr (Kerr-Schild)
  }
}

// A Duration's Debug form with two decimals ({:.2?}, core::time: the largest unit of s /
// ms / us / ns with a non-zero integer part; the dropped digits round half up).
static std::string rust_duration_2(double secs) {
  const unsigned long long ns = (unsigned long long)std::llround(secs * 1e9);
  unsigned long long div;
  const char* unit;
  if (ns >= 1000000000ull) { div = 1000000000ull; unit = "s"; }
  else if (ns >= 1000000ull) { div = 1000000ull; unit = "ms"; }
  else if (ns >= 1000ull) { div = 1000ull; unit = "\u00b5s"; }
  else { div = 1ull; unit = "ns"; }
  if (div == 1) return std::to_string(ns) + ".00" + unit;
  const unsigned long long hundredths = (ns * 100 + div / 2) / div;
  char buf[64];
  std::snprintf(buf, sizeof(buf), "%llu.%02llu%s", hundredths / 100, hundredths % 100, unit);
  return buf;
}

static const char* stop_name(int s) {  // integrator.rs StopReason, as logged by the reference
  switch (s) {
    case GRT_STOP_HORIZON: return "Some(HorizonReached)";
    case GRT_STOP_CELESTIAL: return "Some(CelestialSphereReached)";
    case GRT_STOP_NAN: return "Some(CoordinateIsNan)";
    case GRT_STOP_CLOSED_ORBIT: return "Some(ClosedOrbitDetected)";
    default: return "None";
  }
}

// render-ray / render-ray-at: integrate one ray on the GPU and save its trajectory
// (main.rs:117-171).  The file is created before integrating, as the reference does.
static int trace_and_save(grt_scene* scene, int device, const grt_scene_desc* d, bool camera, const double* a,
                          const double* b, const std::string& filename) {
  FILE* f = std::fopen(filename.c_str(), "wb");
  if (!f) {
    std::fprintf(stderr, "Error: cannot create %s\n", filename.c_str());
    return 1;
  }
  std::fclose(f);
  const uint64_t cap = d->max_steps > 0 ? d->max_steps : 1;  // steps 0 .. max_steps-1
  std::vector<double> steps(cap * 9);
  uint64_t n = 0;
  uint8_t stop = 0, status = 0;
  int rc = camera ? grt_trace_pixels(scene, device, 1, a, b, cap, steps.data(), &n, &stop, &status)
                  : grt_trace_rays(scene, device, 1, a, b, cap, steps.data(), &n, &stop, &status);
  if (rc) {
    std::fprintf(stderr, "Error: %s\n", grt_last_error());
    return 1;
  }
  if (status != GRT_OK) {
    std::fprintf(stderr, "Error: %s\n", status == GRT_ERR_MAX_STEPS_REACHED ? "Max steps reached" : "integration failed");
    return 1;
  }
  std::fprintf(stderr, "[grt] INFO Stop reason: %s\n", stop_name(stop));
  if (grt_write_trajectory_csv(filename.c_str(), d->geometry, d->a, steps.data(), n < cap ? n : cap)) {
    std::fprintf(stderr, "Error: %s\n", grt_last_error());
    return 1;
  }
  std::fprintf(stderr, "[grt] INFO Saved integrated ray to %s\n", filename.c_str());
  return 0;
}

// The log lines of one rendered frame or section (origin r0, c0, width w), as the reference
// prints them.  The 1-spp pass, in pixel order (the reference logs from its parallel loop):
//  * raytracer.rs:232-239: a pixel whose color_of_ray failed (Debug form of the
//    RaytracerError); it keeps the default colour;
//  * scene.rs:178-183 / :196-202: an error-free ray that ended on NaN coordinates or
//    without a terminal event (steps.len() counts the initial step too).
// Then, with `supersampled`, supersample's line (raytracer.rs:325) and its sub-rays' lines.
static void log_frame_rays(uint32_t r0, uint32_t c0, uint32_t w, const std::vector<uint8_t>& status,
                           const std::vector<uint8_t>& stop, const std::vector<uint32_t>& steps, bool supersampled,
                           uint64_t nsel, const grt_subsample_failures& fails) {
  for (size_t i = 0; i < status.size(); ++i) {
    const unsigned col = (unsigned)(c0 + i % w), row = (unsigned)(r0 + i / w);
    if (status[i] & 0x7f)
      std::fprintf(stderr, "[grt] ERROR Unable to compute color for ray at pixel (%u, %u): %s\n", col, row,
                   error_debug_name(status[i] & 0x7f));
    else
      log_ray_event(row, col, stop[i], steps[i]);
  }
  if (!supersampled) return;
  std::fprintf(stderr, "[grt] INFO Supersampling %llu pixels\n", (unsigned long long)nsel);
  // :357-362: the same error line for each failed sub-sample ray of a supersampled pixel
  for (uint64_t k = 0; k < std::min<uint64_t>(fails.count, fails.capacity); ++k) {
    const unsigned col = (unsigned)(c0 + fails.pixel[k] % w), row = (unsigned)(r0 + fails.pixel[k] / w);
    if (fails.status[k])
      std::fprintf(stderr, "[grt] ERROR Unable to compute color for ray at pixel (%u, %u): %s\n", col, row,
                   error_debug_name(fails.status[k]));
    else
      log_ray_event(row, col, fails.stop[k], fails.steps[k]);
  }
  if (fails.count > fails.capacity)
    std::fprintf(stderr, "[grt] ERROR %llu more failed or unterminated sub-sample rays not listed\n",
                 (unsigned long long)(fails.count - fails.capacity));
}

// The output stage of a frame: `.hdr` (f32 XYZ) or the tone-mapped PNG by the extension of
// `filename`, and the raw f64 XYZA dump when asked for.  Adds its times to *ph_output (tone
// map) and *ph_write (encode + write).  Returns 0 or the process exit code.
static int write_frame(const std::string& filename, const std::string& raw_out, const std::vector<double>& xyza,
                       uint32_t w, uint32_t h, int32_t tone_mapping, int device, double* ph_output, double* ph_write) {
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  const bool hdr = filename.size() >= 4 && filename.compare(filename.size() - 4, 4, ".hdr") == 0;
  std::string err;
  bool ok;
  auto t_phase = clk::now();
  if (hdr) {
    std::vector<float> rgb((size_t)w * h * 3);
    for (size_t i = 0; i < (size_t)w * h; ++i)
      for (int k = 0; k < 3; ++k) rgb[3 * i + k] = (float)xyza[4 * i + k];
    ok = grt_host::hdr_encode_rgb(filename, rgb.data(), w, h, err);
  } else {
    std::vector<uint8_t> rgb((size_t)w * h * 3);
    // output stage on the GPU (color.rs:204-298 via output.hip), exposure 1 as in
    // render_section (raytracer.rs:485)
    if (grt_xyz_to_srgb8_device(device, xyza.data(), (size_t)w * h, tone_mapping, 1.0, rgb.data())) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    *ph_output += ms_since(t_phase);
    t_phase = clk::now();
    ok = grt_host::png_encode_rgb(filename, rgb.data(), w, h, err);
  }
  if (!ok) {
    std::fprintf(stderr, "Error: %s\n", err.c_str());
    return 1;
  }
  if (!raw_out.empty()) {
    FILE* f = std::fopen(raw_out.c_str(), "wb");
    if (f) {
      std::fwrite(xyza.data(), 8, xyza.size(), f);
      std::fclose(f);
    }
  }
  *ph_write += ms_since(t_phase);
  return 0;
}

// Host arrays of a geometry buffer of n pixels and nl layers (gbuffer, reshade).
struct GBufferHost {
  size_t n, nl;
  std::vector<uint8_t> status, stop, object;
  std::vector<uint32_t> steps;
  std::vector<uint64_t> layer_start;
  std::vector<double> sky, layer;  // [3][n] u, v, redshift; [4][nl] u, v, redshift, radius
  GBufferHost(size_t n_, size_t nl_)
      : n(n_), nl(nl_), status(n_), stop(n_), object(nl_), steps(n_), layer_start(n_ + 1), sky(3 * n_), layer(4 * nl_) {}
  grt_gbuffer_arrays arrays() {
    return grt_gbuffer_arrays{status.data(),        stop.data(),        steps.data(),          sky.data(),
                              sky.data() + n,       sky.data() + 2 * n, layer_start.data(),    object.data(),
                              layer.data(),         layer.data() + nl,  layer.data() + 2 * nl, layer.data() + 3 * nl};
  }
};

// The sub-sample set of a buffer on the host (gbuffer / reshade --adaptive): the sidecar
// `<file>.sub` of grt_gbuffer_sub_write_file.
struct GBufferSubHost {
  grt_gbuffer_sub_info sub;
  std::vector<uint32_t> sub_pixel;
  GBufferHost rays;
  explicit GBufferSubHost(const grt_gbuffer_sub_info& s)
      : sub(s), sub_pixel(s.n_sub_pixels), rays(s.n_sub_rays, s.n_sub_layers) {}
};

// A timed set's lapse goes beside it, to `<path>.lapse` (grt_gbuffer_sub_lapse_write_file).
static int save_sub_sidecar(const grt_gbuffer* gb, const grt_gbuffer_info& info, const std::string& path) {
  grt_gbuffer_sub_info sub;
  if (grt_gbuffer_sub_info_get(gb, &sub)) return 1;
  GBufferSubHost h(sub);
  const grt_gbuffer_arrays arr = h.rays.arrays();
  if (grt_gbuffer_sub_download(gb, h.sub_pixel.data(), &arr) ||
      grt_gbuffer_sub_write_file(path.c_str(), &info, &sub, h.sub_pixel.data(), &arr))
    return 1;
  if (grt_gbuffer_sub_has_lapse(gb) != 1) return 0;
  std::vector<double> lapse(sub.n_sub_layers);
  return grt_gbuffer_sub_lapse_download(gb, lapse.data()) ||
         grt_gbuffer_sub_lapse_write_file((path + ".lapse").c_str(), &info, &sub, lapse.data(), sub.n_sub_layers);
}

static bool file_exists(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (f) std::fclose(f);
  return f != nullptr;
}

// The lapse of the set just loaded from `<sidecar>` (its info `sub`), when `<sidecar>.lapse` is
// there: the set is then a timed one.  A sidecar of another or of a since-grown set fails.
static int load_sub_lapse_sidecar(grt_gbuffer* gb, const grt_gbuffer_info& info, const grt_gbuffer_sub_info& sub,
                                  const std::string& sidecar) {
  const std::string path = sidecar + ".lapse";
  if (!file_exists(path)) return 0;
  std::vector<double> lapse(sub.n_sub_layers);
  if (grt_gbuffer_sub_lapse_read_file(path.c_str(), &info, &sub, lapse.data())) return 1;
  if (sub.samples_per_axis == 0) return 0;  // no set to time
  return grt_gbuffer_sub_lapse_upload(gb, lapse.data(), sub.n_sub_layers);
}

// render-sequence: a camera-path file, one camera per line `x,y,z,phi,theta,psi` (the
// values --camera-position, --phi, --theta, --psi take); blank lines and lines starting
// with `#` are skipped.  On error *err names the line.
static bool load_camera_path(const std::string& path, std::vector<std::vector<double>>& cams, std::string* err) {
  FILE* f = std::fopen(path.c_str(), "r");
  if (!f) {
    *err = "cannot read the camera path " + path;
    return false;
  }
  std::string text;
  char buf[4096];
  size_t got;
  while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
  std::fclose(f);
  size_t no = 0;
  for (size_t p = 0; p < text.size();) {
    size_t q = text.find('\n', p);
    if (q == std::string::npos) q = text.size();
    std::string line = text.substr(p, q - p);
    p = q + 1;
    ++no;
    const size_t a = line.find_first_not_of(" \t\r"), b = line.find_last_not_of(" \t\r");
    if (a == std::string::npos || line[a] == '#') continue;
    line = line.substr(a, b - a + 1);
    std::vector<double> v;
    if (!split_csv(line, v) || v.size() != 6) {
      *err = path + ":" + std::to_string(no) + ": expected six numbers `x,y,z,phi,theta,psi`, found `" + line + "`";
      return false;
    }
    cams.push_back(v);
  }
  if (cams.empty()) {
    *err = path + ":1: the camera path holds no camera";
    return false;
  }
  return true;
}

// `pattern` with its one `%d` / `%0Nd` conversion replaced by `index`; false when the
// pattern has no such conversion (every frame would overwrite the last).
static bool expand_pattern(const std::string& pattern, long long index, std::string* out) {
  const size_t p = pattern.find('%');
  if (p == std::string::npos) return false;
  size_t q = p + 1;
  const bool zero = q < pattern.size() && pattern[q] == '0';
  int width = 0;
  while (q < pattern.size() && std::isdigit((unsigned char)pattern[q])) width = width * 10 + (pattern[q++] - '0');
  if (q >= pattern.size() || pattern[q] != 'd' || width > 32 || pattern.find('%', q) != std::string::npos) return false;
  std::string num = std::to_string(index);
  if ((int)num.size() < width) num.insert(0, (size_t)width - num.size(), zero ? '0' : ' ');
  *out = pattern.substr(0, p) + num + pattern.substr(q + 1);
  return true;
}

int main(int argc, char** argv) {
  auto t_start = std::chrono::steady_clock::now();
  grt_global_opts opts;
  grt_default_global_opts(&opts);
  std::string config_file, action, filename, resource_root, raw_out;
  long from_row = -1, from_col = -1, to_row = -1, to_col = -1;
  long long ray_row = 0, ray_col = 0;
  bool have_row = false, have_col = false;
  std::vector<double> ray_position, ray_direction;
  bool have_position = false, have_direction = false;
  // blackbody / blackbody-spectrum (cli.rs:88-110 defaults)
  double bb_temperature = 0.0, bb_redshift = 1.0, bb_tmin = 1000.0, bb_tmax = 10000.0, bb_zmin = 0.5, bb_zmax = 2.0;
  uint32_t bb_w = 1000, bb_h = 1000;
  bool have_temperature = false;
  int device = 0;
  std::vector<int> multi_devices;  // --gpus / --devices: the multi-GPU frame
  uint32_t band_rows = 16;
  std::string camera_path, filename_pattern = "frame-%04d.png";  // render-sequence
  std::string gbuffer_file;  // reshade
  std::string gbuffer_pattern;  // reshade-sequence
  long long n_frames = -1;      // reshade-sequence --frames
  bool have_pattern = false;    // --filename-pattern given (gbuffer-sequence has no default)
  bool gbuffer_adaptive = false;  // gbuffer / reshade --adaptive: the config's [adaptive_sampling]
  bool seq_adaptive = false;      // gbuffer-sequence / reshade-sequence --adaptive-stacked: the same, stacked
  std::string orbit_times, raw_out_pattern;  // reshade-orbit --times T0,DT,K, --raw-out-pattern
  bool gbuffer_lapse = false;   // gbuffer --lapse: record each layer's light-travel time (F.grtg.lapse)
  bool orbit_retarded = false;  // reshade-orbit --retarded: every disc layer at its emission time
  bool orbit_adaptive_retarded = false;  // reshade-orbit --adaptive-retarded: --adaptive under that rule
  double orbit_t0 = 0.0, orbit_dt = 0.0;
  long long first_index = 0;
  std::vector<std::string> args(argv + 1, argv + argc);
  for (size_t i = 0; i < args.size(); ++i) {
    std::string a = args[i], val;
    bool has_eq = false;
    size_t eq = a.find('=');
    if (a.rfind("--", 0) == 0 && eq != std::string::npos) {
      val = a.substr(eq + 1);
      a = a.substr(0, eq);
      has_eq = true;
    }
    auto next = [&](std::string& v) -> bool {
      if (has_eq) {
        v = val;
        return true;
      }
      if (i + 1 >= args.size()) return false;
      v = args[++i];
      return true;
    };
    std::string v;
    if (action.empty() && (a == "render" || a == "render-sequence" || a == "render-ray" || a == "render-ray-at" ||
                           a == "blackbody" || a == "blackbody-spectrum" || a == "gbuffer" || a == "reshade" ||
                           a == "gbuffer-sequence" || a == "reshade-sequence" || a == "reshade-orbit")) {
      action = a;
      continue;
    }
    if (action.empty() && a == "--show-sampling-mask") { opts.show_sampling_mask = 1; continue; }
    if ((action == "gbuffer" || action == "reshade" || action == "reshade-orbit") && a == "--adaptive") {
      gbuffer_adaptive = true;
      continue;
    }
    if (action == "gbuffer" && a == "--lapse") {
      gbuffer_lapse = true;
      continue;
    }
    if (action == "reshade-orbit" && a == "--adaptive-retarded") {
      orbit_adaptive_retarded = true;
      continue;
    }
    if (action == "reshade-orbit" && a == "--retarded") {
      orbit_retarded = true;
      continue;
    }
    if ((action == "gbuffer-sequence" || action == "reshade-sequence") && a == "--adaptive-stacked") {
      seq_adaptive = true;
      continue;
    }
    if ((action == "gbuffer-sequence" || action == "reshade-sequence") && a == "--adaptive")
      return usage((action + " has no --adaptive: the stacked adaptive frames are --adaptive-stacked; for one frame "
                    "run `gbuffer --adaptive` / `reshade --adaptive` (a sequence's .grtg files are ordinary "
                    "g-buffers)").c_str());
    if (!next(v)) return usage(("missing value for " + a).c_str());
    std::vector<double> nums;
    auto bad = [&]() { return usage(("invalid value '" + v + "' for '" + a + "'").c_str()); };
    auto f64 = [&](double* out) { return parse_f64(v, out); };
    auto int_in = [&](long long lo, unsigned long long hi, long long* out) { return parse_i64(v, lo, hi, out); };
    long long iv = 0;
    // extras accepted anywhere
    if (a == "--device") { device = std::atoi(v.c_str()); continue; }
    if (a == "--gpus") {
      if (!int_in(1, GRT_MULTI_MAX_DEVICES, &iv)) return bad();
      multi_devices.clear();
      for (long long k = 0; k < iv; ++k) multi_devices.push_back((int)k);
      continue;
    }
    if (a == "--devices") {
      std::vector<double> ds;
      if (!split_csv(v, ds) || ds.empty() || ds.size() > GRT_MULTI_MAX_DEVICES) return bad();
      multi_devices.clear();
      for (double x : ds) {
        if (x < 0 || x != (double)(int)x) return bad();
        multi_devices.push_back((int)x);
      }
      continue;
    }
    if (a == "--arithmetic") {
      if (v != "exact" && v != "fused") return bad();
      (void)grt_set_arithmetic(v == "fused" ? 1 : 0);
      continue;
    }
    if (a == "--transport") {
      const int mode = v == "rccl" ? GRT_TRANSPORT_RCCL : v == "peer" ? GRT_TRANSPORT_PEER
                       : v == "peer-staged" ? GRT_TRANSPORT_PEER_STAGED : -1;
      if (mode < 0) return bad();
      (void)grt_set_multi_transport(mode);
      continue;
    }
    if (a == "--band-rows") {
      if (!int_in(1, 4294967295ull, &iv)) return bad();
      band_rows = (uint32_t)iv;
      continue;
    }
    if (a == "--resource-root") { resource_root = v; continue; }
    if (a == "--raw-out") { raw_out = v; continue; }
    if (!action.empty()) {  // subcommand options
      const bool seq_action = action == "render-sequence" || action == "gbuffer-sequence" ||
                              action == "reshade-sequence" || action == "reshade-orbit";
      if (a == "--filename" && !seq_action) filename = v;
      else if ((action == "reshade" || action == "reshade-orbit") && a == "--gbuffer") gbuffer_file = v;
      else if (action == "reshade-orbit" && a == "--times") orbit_times = v;
      else if (action == "reshade-orbit" && a == "--raw-out-pattern") raw_out_pattern = v;
      else if ((action == "render-sequence" || action == "gbuffer-sequence") && a == "--camera-path") camera_path = v;
      else if (seq_action && a == "--filename-pattern") {
        filename_pattern = v;
        have_pattern = true;
      }
      else if (seq_action && a == "--first-index") {
        if (!int_in(0, 1000000000ull, &iv)) return bad();
        first_index = iv;
      }
      else if (action == "reshade-sequence" && a == "--gbuffer-pattern") gbuffer_pattern = v;
      else if (action == "reshade-sequence" && a == "--frames") {
        if (!int_in(0, 4294967295ull, &iv)) return bad();
        n_frames = iv;
      }
      else if (action == "render" && (a == "--from-row" || a == "--from-col" || a == "--to-row" || a == "--to-col")) {
        if (!int_in(0, 4294967295ull, &iv)) return bad();  // Option<u32>
        (a == "--from-row" ? from_row : a == "--from-col" ? from_col : a == "--to-row" ? to_row : to_col) = (long)iv;
      } else if (action == "render-ray" && (a == "-r" || a == "--row")) {
        if (!int_in(INT64_MIN, INT64_MAX, &iv)) return bad();  // i64
        ray_row = iv;
        have_row = true;
      } else if (action == "render-ray" && (a == "-c" || a == "--col")) {
        if (!int_in(INT64_MIN, INT64_MAX, &iv)) return bad();
        ray_col = iv;
        have_col = true;
      }
      else if (action == "render-ray-at" && (a == "-p" || a == "--position")) {
        if (!split_csv(v, ray_position)) return usage("invalid position");
        have_position = true;
      } else if (action == "render-ray-at" && (a == "-d" || a == "--direction")) {
        if (!split_csv(v, ray_direction)) return usage("invalid direction");
        have_direction = true;
      } else if (action == "blackbody" && (a == "-t" || a == "--temperature")) {
        if (!f64(&bb_temperature)) return bad();
        have_temperature = true;
      } else if (action == "blackbody" && (a == "-r" || a == "--redshift")) {
        if (!f64(&bb_redshift)) return bad();
      } else if (action == "blackbody-spectrum" && a == "--min-temperature") {
        if (!f64(&bb_tmin)) return bad();
      } else if (action == "blackbody-spectrum" && a == "--max-temperature") {
        if (!f64(&bb_tmax)) return bad();
      } else if (action == "blackbody-spectrum" && a == "--min-redshift") {
        if (!f64(&bb_zmin)) return bad();
      } else if (action == "blackbody-spectrum" && a == "--max-redshift") {
        if (!f64(&bb_zmax)) return bad();
      } else if (action == "blackbody-spectrum" && (a == "--width" || a == "--height")) {
        if (!int_in(0, 4294967295ull, &iv)) return bad();  // u32
        (a == "--width" ? bb_w : bb_h) = (uint32_t)iv;
      }
      else if (action == "blackbody-spectrum" && a == "-f") filename = v;
      else return usage(("unknown argument " + a + " for " + action).c_str());
      continue;
    }
    if (a == "--width" || a == "--height") {
      if (!int_in(INT64_MIN, INT64_MAX, &iv)) return bad();  // i64
      (a == "--width" ? opts.width : opts.height) = iv;
    } else if (a == "--max-steps") {  // usize
      const std::string d = (!v.empty() && v[0] == '+') ? v.substr(1) : v;
      if (d.empty() || d.find_first_not_of("0123456789") != std::string::npos) return bad();
      errno = 0;
      opts.max_steps = std::strtoull(d.c_str(), nullptr, 10);
      if (errno == ERANGE) return bad();
    } else if (a == "--step-size") { if (!f64(&opts.step_size)) return bad(); }
    else if (a == "--max-radius") { if (!f64(&opts.max_radius)) return bad(); }
    else if (a == "--epsilon") { if (!f64(&opts.epsilon)) return bad(); }
    else if (a == "--phi") { if (!f64(&opts.phi)) return bad(); }
    else if (a == "--theta") { if (!f64(&opts.theta)) return bad(); }
    else if (a == "--psi") { if (!f64(&opts.psi)) return bad(); }
    else if (a == "--camera-position") {
      if (!split_csv(v, nums) || nums.size() != 3) return usage("Camera position must be a vector of length 3");
      for (int k = 0; k < 3; ++k) opts.camera_position[k] = nums[k];
    } else if (a == "--tone-mapping") {
      if (v == "reinhard") opts.tone_mapping = GRT_TONE_REINHARD;
      else if (v == "global-linear") opts.tone_mapping = GRT_TONE_GLOBAL_LINEAR;
      else return usage("tone mapping must be reinhard or global-linear");
    } else if (a == "--sampling-mask-color") {
      uint8_t rgb[3];
      if (!parse_rgb(v, rgb)) return usage(("invalid RGB color '" + v + "'; expected R,G,B").c_str());
      for (int k = 0; k < 3; ++k) opts.sampling_mask_color[k] = rgb[k];
    } else if (a == "-c" || a == "--config-file") config_file = v;
    else return usage(("unknown argument " + a).c_str());
  }
  if (action.empty())
    return usage("missing subcommand (render, render-sequence, render-ray, render-ray-at, gbuffer, reshade, "
                 "gbuffer-sequence, reshade-sequence, reshade-orbit, blackbody, blackbody-spectrum)");
  if (action == "blackbody") {  // run_blackbody (cli/blackbody.rs:7-25): no scene needed
    if (!have_temperature) return usage("blackbody needs --temperature");
    double xyz[3];
    uint8_t c[3];
    grt_blackbody_xyz(bb_temperature, bb_redshift, xyz);
    grt_xyz_to_srgb(xyz, 1.0, c);
    std::printf("Blackbody color at T=%sK (redshift=%s):\n", grt_host::rust_display_f64(bb_temperature).c_str(),
                grt_host::rust_display_f64(bb_redshift).c_str());
    std::printf("XYZ:  %.4f, %.4f, %.4f\n", xyz[0], xyz[1], xyz[2]);
    std::printf("sRGB: R=%u, G=%u, B=%u\n", c[0], c[1], c[2]);
    std::printf("sRGB: R=%.4f, G=%.4f, B=%.4f\n", c[0] / 255.0, c[1] / 255.0, c[2] / 255.0);
    std::printf("Color block: \x1b[48;2;%u;%u;%um      \x1b[0m\n", c[0], c[1], c[2]);
    return 0;
  }
  if (action == "blackbody-spectrum") {  // run_blackbody_spectrum (cli/blackbody.rs:27-95)
    if (filename.empty()) filename = "blackbody_spectrum.png";
    std::vector<uint8_t> rgba((size_t)bb_w * bb_h * 4);
    if (grt_blackbody_spectrum(bb_tmin, bb_tmax, bb_zmin, bb_zmax, bb_w, bb_h, opts.tone_mapping, rgba.data())) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    std::string err;
    if (!grt_host::png_encode_rgba(filename, rgba.data(), bb_w, bb_h, err)) {
      std::fprintf(stderr, "Failed to save spectrum image: %s\n", err.c_str());
      return 1;
    }
    std::printf("Saved blackbody spectrum to %s\n", filename.c_str());
    return 0;
  }
  if (action == "render-ray" && !(have_row && have_col)) return usage("render-ray needs --row and --col");
  if (action == "render-ray-at" && !(have_position && have_direction))
    return usage("render-ray-at needs --position and --direction");
  if (action == "gbuffer" && filename.empty()) return usage("gbuffer needs --filename");
  if (action == "reshade" && gbuffer_file.empty()) return usage("reshade needs --gbuffer");
  // the multi-GPU g-buffer is the 1-spp trace (grt_gbuffer_trace_multi): the sub-rays are a top-up on the buffer's GPU
  if (action == "gbuffer" && gbuffer_adaptive && !multi_devices.empty())
    return usage("gbuffer --adaptive runs on one GPU (--device); --gpus / --devices do not apply: trace with "
                 "`gbuffer --gpus N`, then `reshade --adaptive` tops up the sub-rays on the buffer's GPU");
  if (action == "gbuffer" && gbuffer_lapse && !multi_devices.empty())
    return usage("gbuffer --lapse runs on one GPU (--device); --gpus / --devices do not apply: the multi-GPU buffer "
                 "records no lapse");
  if (action == "reshade" && !multi_devices.empty())
    return usage("reshade runs on one GPU (--device); --gpus / --devices do not apply: trace with `gbuffer --gpus N`, "
                 "then `reshade [--adaptive]` shades (and tops up) on the buffer's GPU");
  if (action == "gbuffer-sequence" || action == "reshade-sequence") {  // every usage error before the GPU is touched
    std::string probe;
    if (!multi_devices.empty())
      return usage((action + " runs on one GPU (--device); --gpus / --devices do not apply: a single frame traces with "
                    "`gbuffer --gpus N`, then `reshade --adaptive` tops up on the buffer's GPU").c_str());
    if (action == "gbuffer-sequence" && camera_path.empty()) return usage("gbuffer-sequence needs --camera-path");
    if (action == "gbuffer-sequence" && !have_pattern)
      return usage("gbuffer-sequence needs --filename-pattern (a-%04d.grtg)");
    if (action == "reshade-sequence" && gbuffer_pattern.empty()) return usage("reshade-sequence needs --gbuffer-pattern");
    if (action == "reshade-sequence" && n_frames < 0) return usage("reshade-sequence needs --frames");
    if (action == "reshade-sequence" && n_frames == 0) return usage("--frames must be at least 1");
    if (action == "reshade-sequence" && !expand_pattern(gbuffer_pattern, first_index, &probe))
      return usage("--gbuffer-pattern needs one %d or %0Nd conversion for the frame index");
    if (!expand_pattern(filename_pattern, first_index, &probe))
      return usage("--filename-pattern needs one %d or %0Nd conversion for the frame index");
    if (action == "reshade-sequence" && !raw_out.empty() && !expand_pattern(raw_out, first_index, &probe))
      return usage("--raw-out of reshade-sequence is a pattern: it needs one %d or %0Nd conversion");
  }
  if (action == "reshade-orbit") {  // every usage error before the GPU is touched
    std::string probe;
    std::vector<double> t;
    if (gbuffer_file.empty()) return usage("reshade-orbit needs --gbuffer");
    if (!multi_devices.empty()) return usage("reshade-orbit runs on one GPU (--device); --gpus / --devices do not apply");
    if (orbit_times.empty()) return usage("reshade-orbit needs --times T0,DT,K");
    if (!split_csv(orbit_times, t) || t.size() != 3 || !std::isfinite(t[0]) || !std::isfinite(t[1]) ||
        !(t[2] >= 0.0 && t[2] <= 4294967295.0) || t[2] != std::floor(t[2]))
      return usage("--times must be T0,DT,K: two finite numbers and a frame count");
    if (t[2] == 0.0) return usage("--times: K must be at least 1");
    if (!std::isfinite(t[0] + (t[2] - 1.0) * t[1])) return usage("--times: the last frame's time is not finite");
    orbit_t0 = t[0];
    orbit_dt = t[1];
    n_frames = (long long)t[2];
    if (!have_pattern) return usage("reshade-orbit needs --filename-pattern (f-%04d.png)");
    if (!expand_pattern(filename_pattern, first_index, &probe))
      return usage("--filename-pattern needs one %d or %0Nd conversion for the frame index");
    if (!raw_out_pattern.empty() && !expand_pattern(raw_out_pattern, first_index, &probe))
      return usage("--raw-out-pattern needs one %d or %0Nd conversion for the frame index");
    if (!raw_out.empty()) return usage("reshade-orbit writes many frames: give --raw-out-pattern, not --raw-out");
    if (orbit_retarded && gbuffer_adaptive)
      return usage("reshade-orbit --retarded does not combine with --adaptive: --retarded shades the 1-spp frames; "
                   "the adaptive frames under the retarded rule are --adaptive-retarded");
    if (orbit_adaptive_retarded && (gbuffer_adaptive || orbit_retarded))
      return usage("reshade-orbit --adaptive-retarded does not combine with --adaptive or --retarded: it is the "
                   "adaptive frame under the retarded rule by itself");
    if ((orbit_retarded || orbit_adaptive_retarded) && !file_exists(gbuffer_file + ".lapse"))  // the lapse's sidecar
      return usage(("reshade-orbit " + std::string(orbit_retarded ? "--retarded" : "--adaptive-retarded") +
                    " needs the lapse sidecar " + gbuffer_file + ".lapse (trace with `gbuffer --lapse`)").c_str());
    if (orbit_adaptive_retarded && file_exists(gbuffer_file + ".sub") && !file_exists(gbuffer_file + ".sub.lapse"))
      return usage(("reshade-orbit --adaptive-retarded: the sub-sample set " + gbuffer_file + ".sub has no lapse sidecar " +
                    gbuffer_file + ".sub.lapse: remove it (its sub-rays are then traced again, timed) or re-run "
                    "`gbuffer --adaptive --lapse`").c_str());
  }
  if (filename.empty())
    filename = (action == "render" || action == "reshade") ? "render.png" : (action == "render-ray" ? "rendered-ray.csv" : "rendered-ray-at.csv");
  if (config_file.empty()) return usage("Config file is required for this action");
  std::vector<std::vector<double>> path_cams;  // render-sequence: x, y, z, phi, theta, psi per frame
  if (action == "render-sequence") {  // every usage error before the GPU is touched
    if (camera_path.empty()) return usage("render-sequence needs --camera-path");
    if (!multi_devices.empty()) return usage("render-sequence runs on one GPU (--device); --gpus / --devices do not apply");
    std::string probe, perr;
    if (!expand_pattern(filename_pattern, first_index, &probe))
      return usage("--filename-pattern needs one %d or %0Nd conversion for the frame index");
    if (!raw_out.empty() && !expand_pattern(raw_out, first_index, &probe))
      return usage("--raw-out of render-sequence is a pattern: it needs one %d or %0Nd conversion");
    if (!load_camera_path(camera_path, path_cams, &perr)) return usage(perr.c_str());
  }
  if (action == "gbuffer-sequence") {
    std::string perr;
    if (config_file.empty()) return usage("Config file is required for this action");
    if (!load_camera_path(camera_path, path_cams, &perr)) return usage(perr.c_str());
  }

  grt_gbuffer_info gb_info, gb_first;
  std::memset(&gb_first, 0, sizeof(gb_first));
  if (action == "reshade-sequence") {  // every file's header and length, before the GPU is touched
    for (long long k = 0; k < n_frames; ++k) {
      std::string name;
      (void)expand_pattern(gbuffer_pattern, first_index + k, &name);
      if (grt_gbuffer_read_file(name.c_str(), &gb_info, nullptr)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      if (gb_info.row0 != 0 || gb_info.col0 != 0 || (int64_t)gb_info.rows != gb_info.camera.rows ||
          (int64_t)gb_info.cols != gb_info.camera.cols) {
        std::fprintf(stderr, "Error: %s holds a rectangle, not a whole frame\n", name.c_str());
        return 1;
      }
      if ((int64_t)gb_info.cols != opts.width || (int64_t)gb_info.rows != opts.height)
        return usage(("--width / --height must be the frame of " + name + ", " + std::to_string(gb_info.cols) + " x " +
                      std::to_string(gb_info.rows)).c_str());
      if (k == 0) gb_first = gb_info;
      // --adaptive-stacked: one tracer serves every frame, so the files' recorded integration parameters agree
#define GRT_SAME(field)                                                                                         \
  if (seq_adaptive && std::memcmp(&gb_info.field, &gb_first.field, sizeof(gb_info.field)) != 0)                 \
    return usage(("--adaptive-stacked: " + name + " differs from the first file in " #field).c_str());
      GRT_SAME(max_steps) GRT_SAME(max_radius) GRT_SAME(step_size) GRT_SAME(epsilon) GRT_SAME(horizon_epsilon)
#undef GRT_SAME
    }
  }
  if (action == "reshade" || action == "reshade-orbit") {  // the file's header and length, before the GPU is touched
    if (config_file.empty()) return usage("Config file is required for this action");
    if (grt_gbuffer_read_file(gbuffer_file.c_str(), &gb_info, nullptr)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    if (gb_info.row0 != 0 || gb_info.col0 != 0 || (int64_t)gb_info.rows != gb_info.camera.rows ||
        (int64_t)gb_info.cols != gb_info.camera.cols) {
      std::fprintf(stderr, "Error: %s holds a rectangle, not a whole frame\n", gbuffer_file.c_str());
      return 1;
    }
    if ((int64_t)gb_info.cols != opts.width || (int64_t)gb_info.rows != opts.height)
      return usage(("--width / --height must be the g-buffer's frame, " + std::to_string(gb_info.cols) + " x " +
                    std::to_string(gb_info.rows)).c_str());
    // the lapse's sidecar: its header, its binding to this buffer and its entries
    if ((orbit_retarded || orbit_adaptive_retarded) &&
        grt_gbuffer_lapse_read_file((gbuffer_file + ".lapse").c_str(), &gb_info, nullptr)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    // and the set's two sidecars: their headers, lengths and bindings, the lapse's entries
    if (orbit_adaptive_retarded && file_exists(gbuffer_file + ".sub")) {
      grt_gbuffer_sub_info held;
      if (grt_gbuffer_sub_read_file((gbuffer_file + ".sub").c_str(), &gb_info, &held, nullptr, nullptr) ||
          grt_gbuffer_sub_lapse_read_file((gbuffer_file + ".sub.lapse").c_str(), &gb_info, &held, nullptr)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
    }
  }

  if (action == "render" && !multi_devices.empty() &&
      (from_row > 0 || from_col > 0 || (to_row >= 0 && to_row != (long long)opts.height) ||
       (to_col >= 0 && to_col != (long long)opts.width)))
    return usage("--gpus / --devices render whole frames (no --from-row/--from-col/--to-row/--to-col)");

  // The HIP runtime's start-up (driver and device enumeration) runs beside the scene load
  // below: the first HIP call of the process does it, wherever it is made.
  std::thread hip_init([] { (void)grt_device_count(); });
  // on every way out of main from here: the start-up thread joined, then the multi-GPU
  // frame's RCCL set-up waited for and torn down (a communicator still being created when
  // the process exits brings the exit down)
  struct Joiner {
    std::thread& t;
    bool multi;
    ~Joiner() {
      if (t.joinable()) t.join();
      if (multi) grt_multi_release();
    }
  } hip_init_join{hip_init, !multi_devices.empty()};
  // phase times of a render (printed on one [grt] line at the end; not in the reference)
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); };
  double ph_load = 0, ph_create = 0, ph_init = 0, ph_render = 0, ph_output = 0, ph_write = 0;
  auto t_phase = clk::now();
  grt_host_scene* hs = nullptr;
  if (action == "render-ray-at" ? grt_host_geometry_load(config_file.c_str(), &opts, &hs)
                                : grt_host_scene_load(config_file.c_str(),
                                                      resource_root.empty() ? nullptr : resource_root.c_str(), &opts,
                                                      &hs)) {
    std::fprintf(stderr, "Error: %s\n", grt_last_error());
    return 1;
  }
  grt_adaptive_config ac;
  grt_host_scene_adaptive(hs, &ac);
  ph_load = ms_since(t_phase);
  t_phase = clk::now();
  grt_scene* scene = nullptr;
  if (grt_scene_create(grt_host_scene_desc(hs), &scene)) {
    std::fprintf(stderr, "Error: %s\n", grt_last_error());
    return 1;
  }
  ph_create = ms_since(t_phase);
  t_phase = clk::now();
  hip_init.join();  // what is left of the HIP runtime's start-up after the load
  ph_init = ms_since(t_phase);
  const grt_scene_desc* d = grt_host_scene_desc(hs);
  auto elapsed = [&]() {  // main.rs:175-176
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
    std::fprintf(stderr, "[grt] INFO Elapsed time: %s\n", rust_duration_2(secs).c_str());
  };
  if (action == "render" || action == "render-sequence")  // main.rs:100-103
    std::fprintf(stderr, "[grt] INFO Using coordinate system: %s\n", coordinate_system_debug(d).c_str());
  {  // the scene setup's info lines (KerrTemperatureComputer::new, temperature.rs:55-102)
    const std::string log = grt_host_scene_log(hs);
    for (size_t p = 0; p < log.size();) {
      size_t q = log.find('\n', p);
      if (q == std::string::npos) q = log.size();
      std::fprintf(stderr, "[grt] INFO %s\n", log.substr(p, q - p).c_str());
      p = q + 1;
    }
  }
  if (action == "gbuffer") {  // trace the frame once at 1 spp, keep its geometry buffer
    grt_gbuffer* gb = nullptr;
    grt_stats st;
    t_phase = clk::now();
    grt_gbuffer_multi_report grep;
    const bool multi = !multi_devices.empty();
    if ((multi ? grt_gbuffer_trace_multi(scene, (int)multi_devices.size(), multi_devices.data(), band_rows, &gb, &st, &grep)
               : (gbuffer_lapse ? grt_gbuffer_trace_lapse : grt_gbuffer_trace)(scene, device, 0, 0, (uint32_t)opts.height,
                                                                               (uint32_t)opts.width, &gb, &st)) ||
        grt_gbuffer_info_get(gb, &gb_info)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    if (multi) {
      for (uint32_t k = 0; k < grep.n_devices; ++k)
        std::fprintf(stderr, "[grt] rank %u (GPU %d): %llu rows, %llu layers, %u trace(s), trace %.1f ms, scan + fill %.2f ms\n",
                     k, multi_devices[k], (unsigned long long)grep.rows[k], (unsigned long long)grep.layers[k],
                     grep.n_traces[k], grep.trace_ms[k], grep.fill_ms[k]);
      std::fprintf(stderr, "[grt] %u GPU(s); transport %s, gather %.2f ms\n", grep.n_devices,
                   transport_name(grep.transport), grep.gather_ms);
    }
    grt_gbuffer_section_report srep;
    if (gbuffer_adaptive && gbuffer_lapse) {
      // the same selection's sub-rays with their lapses, a timed set: the mask pass paints the
      // selected pixels and traces nothing (no shaded pixel has the paint's alpha of -1), then
      // grt_gbuffer_supersample_lapse appends them in the order the top-up below would
      std::memset(&srep, 0, sizeof(srep));
      if (ac.enabled) {
        const double paint[4] = {-1.0, -1.0, -1.0, -1.0};
        std::vector<double> frame(4 * (size_t)gb_info.n_pixels);
        std::vector<uint32_t> px;
        if (grt_gbuffer_shade_section(scene, gb, &ac, paint, nullptr, frame.data(), nullptr, nullptr, nullptr, nullptr,
                                      nullptr)) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        for (size_t p = 0; p < (size_t)gb_info.n_pixels; ++p)
          if (frame[4 * p + 3] == -1.0) px.push_back((uint32_t)p);
        if (grt_gbuffer_supersample_lapse(scene, gb, ac.samples_per_axis, px.size(), px.data(), &srep.top_up)) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        srep.n_selected = srep.n_traced = px.size();
        srep.trace_ms = srep.top_up.kernel_ms;
      }
    } else if (gbuffer_adaptive) {  // this scene's own adaptive frame: the buffer then holds its selection's sub-rays
      std::vector<double> frame(4 * (size_t)gb_info.n_pixels);
      if (grt_gbuffer_shade_section(scene, gb, &ac, nullptr, scene, frame.data(), nullptr, nullptr, nullptr, nullptr,
                                    &srep)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
    }
    ph_render = ms_since(t_phase);
    t_phase = clk::now();
    const size_t n = gb_info.n_pixels, nl = gb_info.n_layers;
    GBufferHost host(n, nl);
    const grt_gbuffer_arrays arr = host.arrays();
    double times[2] = {0, 0};
    (void)grt_gbuffer_trace_times(gb, times);
    if (grt_gbuffer_download(gb, &arr) || grt_gbuffer_write_file(filename.c_str(), &gb_info, &arr) ||
        (gbuffer_adaptive && save_sub_sidecar(gb, gb_info, filename + ".sub"))) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    if (gbuffer_lapse) {  // the layers' light-travel times, beside the file
      std::vector<double> lapse(nl);
      if (grt_gbuffer_lapse_download(gb, lapse.data()) ||
          grt_gbuffer_lapse_write_file((filename + ".lapse").c_str(), &gb_info, lapse.data(), nl)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      std::fprintf(stderr, "[grt] INFO saved lapse to %s.lapse\n", filename.c_str());
      if (gbuffer_adaptive) {
        if (grt_gbuffer_sub_has_lapse(gb) != 1) {  // no set (adaptive sampling is off): an empty sidecar beside the empty .sub
          grt_gbuffer_sub_info none;
          if (grt_gbuffer_sub_info_get(gb, &none) ||
              grt_gbuffer_sub_lapse_write_file((filename + ".sub.lapse").c_str(), &gb_info, &none, nullptr, 0)) {
            std::fprintf(stderr, "Error: %s\n", grt_last_error());
            return 1;
          }
        }
        std::fprintf(stderr, "[grt] INFO saved sub-sample lapse to %s.sub.lapse\n", filename.c_str());
      }
    }
    if (gbuffer_adaptive)
      std::fprintf(stderr, "[grt] sub-sample set: %llu selected pixels traced (%llu sub-rays, %.1f ms), saved to %s.sub\n",
                   (unsigned long long)srep.n_traced, (unsigned long long)srep.top_up.rays, srep.trace_ms,
                   filename.c_str());
    ph_write = ms_since(t_phase);
    std::fprintf(stderr, "[grt] %llu rays, %llu accepted steps, %llu attempts, kernel %.1f ms; g-buffer: %llu layers, "
                 "scan + fill %.2f ms\n", (unsigned long long)st.rays, (unsigned long long)st.accepted_steps,
                 (unsigned long long)st.attempts, st.kernel_ms, (unsigned long long)nl, times[1]);
    std::fprintf(stderr, "[grt] INFO saved g-buffer to %s\n", filename.c_str());
    std::fprintf(stderr, "[grt] phases (ms): load %.1f, create %.1f, hip init %.1f, render %.1f, output %.1f, "
                 "write %.1f, since start %.1f\n", ph_load, ph_create, ph_init, ph_render, ph_output, ph_write,
                 ms_since(t_start));
    elapsed();
    grt_gbuffer_destroy(gb);
    grt_scene_destroy(scene);
    grt_host_scene_destroy(hs);
    return 0;
  }
  if (action == "reshade") {  // the traced frame under this config's appearance
    const size_t n = gb_info.n_pixels, nl = gb_info.n_layers;
    GBufferHost host(n, nl);
    const grt_gbuffer_arrays arr = host.arrays();
    grt_gbuffer* gb = nullptr;
    std::vector<float> x32(4 * n);
    std::vector<uint8_t> cls(n), status(n);
    std::vector<double> xyza(4 * n);
    float shade_ms = 0;
    t_phase = clk::now();
    if (grt_gbuffer_read_file(gbuffer_file.c_str(), &gb_info, &arr) || grt_gbuffer_upload(&gb_info, &arr, device, &gb)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    grt_scene* tracer = nullptr;
    grt_gbuffer_section_report srep;
    uint64_t nsel = 0;
    const uint64_t fail_cap = gbuffer_adaptive ? 1u << 20 : 0;
    std::vector<uint32_t> fail_pix(fail_cap), fail_sample(fail_cap), fail_steps(fail_cap);
    std::vector<uint8_t> fail_status(fail_cap), fail_stop(fail_cap);
    grt_subsample_failures fails{fail_cap, fail_pix.data(), fail_sample.data(), fail_status.data(), 0,
                                 fail_stop.data(), fail_steps.data()};
    double mask[4];
    const double* maskp = nullptr;
    if (gbuffer_adaptive) {
      // this config's scene with the file's recorded camera and integration parameters: it
      // traces the sub-rays the set does not hold yet, and its appearance is the one applied
      grt_scene_desc td = *d;
      td.camera = gb_info.camera;
      td.max_steps = gb_info.max_steps;
      td.max_radius = gb_info.max_radius;
      td.step_size = gb_info.step_size;
      td.epsilon = gb_info.epsilon;
      td.horizon_epsilon = gb_info.horizon_epsilon;
      if (grt_scene_create(&td, &tracer)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      const std::string sidecar = gbuffer_file + ".sub";
      grt_gbuffer_sub_info before;
      std::memset(&before, 0, sizeof(before));
      if (FILE* f = std::fopen(sidecar.c_str(), "rb")) {  // the sidecar, if present
        std::fclose(f);
        if (grt_gbuffer_sub_read_file(sidecar.c_str(), &gb_info, &before, nullptr, nullptr)) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        GBufferSubHost h(before);
        const grt_gbuffer_arrays sarr = h.rays.arrays();
        if (grt_gbuffer_sub_read_file(sidecar.c_str(), &gb_info, &before, h.sub_pixel.data(), &sarr) ||
            grt_gbuffer_sub_upload(gb, &before, h.sub_pixel.data(), &sarr) ||
            load_sub_lapse_sidecar(gb, gb_info, before, sidecar)) {  // with its lapse the set stays timed
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
      }
      if (opts.show_sampling_mask) {
        grt_srgb_to_xyza(opts.sampling_mask_color[0], opts.sampling_mask_color[1], opts.sampling_mask_color[2], 255, mask);
        maskp = mask;
      }
      if (grt_gbuffer_shade_section(tracer, gb, &ac, maskp, tracer, xyza.data(), cls.data(), status.data(), &nsel, &fails,
                                    &srep)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      shade_ms = (float)srep.shade_ms;
      log_frame_rays(0, 0, gb_info.cols, status, host.stop, host.steps, ac.enabled && !maskp, nsel, fails);
      std::fprintf(stderr, "[grt] adaptive re-shade: %llu selected pixels, %llu held, %llu traced (%llu sub-rays, %.1f ms)\n",
                   (unsigned long long)srep.n_selected, (unsigned long long)srep.n_held,
                   (unsigned long long)srep.n_traced, (unsigned long long)srep.top_up.rays, srep.trace_ms);
      grt_gbuffer_sub_info after;
      if (grt_gbuffer_sub_info_get(gb, &after)) return 1;
      if (after.n_sub_pixels > before.n_sub_pixels) {  // the set grew: the next re-shade finds it
        if (save_sub_sidecar(gb, gb_info, sidecar)) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        std::fprintf(stderr, "[grt] INFO saved sub-sample set to %s\n", sidecar.c_str());
      }
    } else if (grt_gbuffer_shade(scene, gb, x32.data(), cls.data(), status.data(), xyza.data(), &shade_ms)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    ph_render = ms_since(t_phase);
    const bool hdr = filename.size() >= 4 && filename.compare(filename.size() - 4, 4, ".hdr") == 0;
    if (hdr) {
      std::fprintf(stderr, "[grt] INFO Creating HDR image\n");
    } else {
      std::fprintf(stderr, "[grt] INFO Creating non-HDR image\n");
      std::fprintf(stderr, "[grt] INFO Tone mapping method: %s\n",
                   opts.tone_mapping == GRT_TONE_GLOBAL_LINEAR ? "GlobalLinear" : "Reinhard");
    }
    std::fprintf(stderr, "[grt] re-shaded %llu pixels, %llu layers from %s, kernel %.2f ms\n", (unsigned long long)n,
                 (unsigned long long)nl, gbuffer_file.c_str(), shade_ms);
    if (int wrc = write_frame(filename, raw_out, xyza, gb_info.cols, gb_info.rows, opts.tone_mapping, device, &ph_output,
                              &ph_write))
      return wrc;
    std::fprintf(stderr, "[grt] INFO saved image to %s\n", filename.c_str());
    std::fprintf(stderr, "[grt] phases (ms): load %.1f, create %.1f, hip init %.1f, render %.1f, output %.1f, "
                 "write %.1f, since start %.1f\n", ph_load, ph_create, ph_init, ph_render, ph_output, ph_write,
                 ms_since(t_start));
    elapsed();
    grt_gbuffer_destroy(gb);
    if (tracer) grt_scene_destroy(tracer);
    grt_scene_destroy(scene);
    grt_host_scene_destroy(hs);
    return 0;
  }
  if (action == "reshade-orbit") {  // one traced frame at K times under this config's appearance
    const uint32_t K = (uint32_t)n_frames;
    const bool adaptive = gbuffer_adaptive || orbit_adaptive_retarded;  // the adaptive frames, under either rule
    const size_t n = gb_info.n_pixels, nl = gb_info.n_layers;
    GBufferHost host(n, nl);
    const grt_gbuffer_arrays arr = host.arrays();
    grt_gbuffer* gb = nullptr;
    t_phase = clk::now();
    if (grt_gbuffer_read_file(gbuffer_file.c_str(), &gb_info, &arr) || grt_gbuffer_upload(&gb_info, &arr, device, &gb)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    std::vector<double> times(K);
    for (uint32_t k = 0; k < K; ++k) times[k] = orbit_t0 + (double)k * orbit_dt;
    std::vector<double> xyza(n * 4 * K);
    float shade_ms = 0;
    grt_scene* tracer = nullptr;
    std::vector<uint8_t> status(adaptive ? n * K : 0);
    std::vector<uint64_t> nsel(K, 0);
    const uint64_t fail_cap = adaptive ? 1u << 16 : 0;  // failed sub-rays logged per frame
    std::vector<uint32_t> fail_pix(fail_cap * K), fail_sample(fail_cap * K), fail_steps(fail_cap * K);
    std::vector<uint8_t> fail_status(fail_cap * K), fail_stop(fail_cap * K);
    std::vector<grt_subsample_failures> fails(K);
    double mask[4];
    const double* maskp = nullptr;
    if (orbit_retarded || orbit_adaptive_retarded) {  // the buffer's lapse from its sidecar (checked before the GPU was touched)
      std::vector<double> lapse(nl);
      if (grt_gbuffer_lapse_read_file((gbuffer_file + ".lapse").c_str(), &gb_info, lapse.data()) ||
          grt_gbuffer_lapse_upload(gb, lapse.data(), nl)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
    }
    if (adaptive) {
      // as `reshade --adaptive`: this config's scene with the file's recorded camera and
      // integration parameters is the appearance and the tracer of the missing sub-rays
      grt_scene_desc td = *d;
      td.camera = gb_info.camera;
      td.max_steps = gb_info.max_steps;
      td.max_radius = gb_info.max_radius;
      td.step_size = gb_info.step_size;
      td.epsilon = gb_info.epsilon;
      td.horizon_epsilon = gb_info.horizon_epsilon;
      if (grt_scene_create(&td, &tracer)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      const std::string sidecar = gbuffer_file + ".sub";
      grt_gbuffer_sub_info before;
      std::memset(&before, 0, sizeof(before));
      if (FILE* f = std::fopen(sidecar.c_str(), "rb")) {  // the sidecar, if present
        std::fclose(f);
        if (grt_gbuffer_sub_read_file(sidecar.c_str(), &gb_info, &before, nullptr, nullptr)) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        GBufferSubHost h(before);
        const grt_gbuffer_arrays sarr = h.rays.arrays();
        if (grt_gbuffer_sub_read_file(sidecar.c_str(), &gb_info, &before, h.sub_pixel.data(), &sarr) ||
            grt_gbuffer_sub_upload(gb, &before, h.sub_pixel.data(), &sarr) ||
            load_sub_lapse_sidecar(gb, gb_info, before, sidecar)) {  // with its lapse the set stays timed
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
      }
      if (opts.show_sampling_mask) {
        grt_srgb_to_xyza(opts.sampling_mask_color[0], opts.sampling_mask_color[1], opts.sampling_mask_color[2], 255, mask);
        maskp = mask;
      }
      for (uint32_t k = 0; k < K; ++k) {  // the frames one after the other: each may top the set up
        fails[k] = grt_subsample_failures{fail_cap, fail_pix.data() + fail_cap * k, fail_sample.data() + fail_cap * k,
                                          fail_status.data() + fail_cap * k, 0, fail_stop.data() + fail_cap * k,
                                          fail_steps.data() + fail_cap * k};
        grt_gbuffer_section_report srep;
        if ((orbit_adaptive_retarded ? grt_gbuffer_shade_section_at_retarded : grt_gbuffer_shade_section_at)(
                tracer, gb, &ac, maskp, tracer, xyza.data() + n * 4 * k, nullptr, status.data() + n * k, &nsel[k],
                &fails[k], &srep, times[k])) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        shade_ms += (float)srep.shade_ms;
        std::fprintf(stderr, "[grt] adaptive re-shade, frame %u (t = %s): %llu selected pixels, %llu held, %llu traced "
                     "(%llu sub-rays, %.1f ms)\n", k, grt_host::rust_display_f64(times[k]).c_str(),
                     (unsigned long long)srep.n_selected, (unsigned long long)srep.n_held,
                     (unsigned long long)srep.n_traced, (unsigned long long)srep.top_up.rays, srep.trace_ms);
      }
      grt_gbuffer_sub_info after;
      if (grt_gbuffer_sub_info_get(gb, &after)) return 1;
      if (after.n_sub_pixels > before.n_sub_pixels) {  // the set grew: the next re-shade finds it
        if (save_sub_sidecar(gb, gb_info, sidecar)) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        std::fprintf(stderr, "[grt] INFO saved sub-sample set to %s\n", sidecar.c_str());
      }
    } else {
      grt_frame_out fo{nullptr, xyza.data(), nullptr, nullptr, nullptr, nullptr};
      if ((orbit_retarded ? grt_gbuffer_shade_times_retarded : grt_gbuffer_shade_times)(scene, gb, K, times.data(), &fo,
                                                                                        &shade_ms)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
    }
    ph_render = ms_since(t_phase);
    std::fprintf(stderr, "[grt] re-shaded %llu pixels, %llu layers from %s at %u times, kernel %.2f ms\n",
                 (unsigned long long)n, (unsigned long long)nl, gbuffer_file.c_str(), K, shade_ms);
    for (uint32_t k = 0; k < K; ++k) {  // each frame tone-mapped on its own, as `reshade` does
      std::string name, raw;
      (void)expand_pattern(filename_pattern, first_index + k, &name);
      if (!raw_out_pattern.empty()) (void)expand_pattern(raw_out_pattern, first_index + k, &raw);
      const bool hdr = name.size() >= 4 && name.compare(name.size() - 4, 4, ".hdr") == 0;
      if (hdr) {
        std::fprintf(stderr, "[grt] INFO Creating HDR image\n");
      } else {
        std::fprintf(stderr, "[grt] INFO Creating non-HDR image\n");
        std::fprintf(stderr, "[grt] INFO Tone mapping method: %s\n",
                     opts.tone_mapping == GRT_TONE_GLOBAL_LINEAR ? "GlobalLinear" : "Reinhard");
      }
      if (adaptive) {  // the frame's ray log, as `reshade --adaptive` writes it
        const std::vector<uint8_t> f_status(status.begin() + n * k, status.begin() + n * (k + 1));
        log_frame_rays(0, 0, gb_info.cols, f_status, host.stop, host.steps, ac.enabled && !maskp, nsel[k], fails[k]);
      }
      const std::vector<double> f_xyza(xyza.begin() + n * 4 * k, xyza.begin() + n * 4 * (k + 1));
      if (int wrc = write_frame(name, raw, f_xyza, gb_info.cols, gb_info.rows, opts.tone_mapping, device, &ph_output,
                                &ph_write))
        return wrc;
      std::fprintf(stderr, "[grt] INFO saved image to %s\n", name.c_str());
    }
    std::fprintf(stderr, "[grt] phases (ms): load %.1f, create %.1f, hip init %.1f, render %.1f, output %.1f, "
                 "write %.1f, since start %.1f\n", ph_load, ph_create, ph_init, ph_render, ph_output, ph_write,
                 ms_since(t_start));
    elapsed();
    grt_gbuffer_destroy(gb);
    if (tracer) grt_scene_destroy(tracer);
    grt_scene_destroy(scene);
    grt_host_scene_destroy(hs);
    return 0;
  }
  if (action == "gbuffer-sequence") {  // the camera path traced stacked, one .grtg per camera
    const uint32_t K = (uint32_t)path_cams.size();
    std::vector<grt_camera_desc> cams(K);
    for (uint32_t k = 0; k < K; ++k) {
      const std::vector<double>& c = path_cams[k];
      if (grt_host_scene_camera(hs, c.data(), c[3], c[4], c[5], &cams[k])) {
        std::fprintf(stderr, "Error: camera %u of %s: %s\n", k, camera_path.c_str(), grt_last_error());
        return 1;
      }
    }
    std::vector<grt_gbuffer*> gbs(K, nullptr);
    grt_stats st;
    grt_gbuffer_sequence_report rep;
    t_phase = clk::now();
    if (grt_gbuffer_trace_sequence(scene, device, K, cams.data(), gbs.data(), &st, &rep)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    grt_gbuffer_section_sequence_report srep;
    std::vector<uint64_t> per_frame(4 * (size_t)K, 0);
    if (seq_adaptive) {  // this scene's own adaptive frames: each buffer then holds its selection's sub-rays
      std::vector<double> frames(4 * (size_t)opts.width * opts.height * K);
      grt_frame_out fo{nullptr, frames.data(), nullptr, nullptr, nullptr, nullptr};
      if (grt_gbuffer_shade_section_sequence(scene, K, gbs.data(), &ac, nullptr, scene, &fo, nullptr, nullptr,
                                             per_frame.data(), &srep)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
    }
    ph_render = ms_since(t_phase);
    t_phase = clk::now();
    unsigned long long layers = 0;
    for (uint32_t k = 0; k < K; ++k) {
      std::string name;
      (void)expand_pattern(filename_pattern, first_index + k, &name);
      if (grt_gbuffer_info_get(gbs[k], &gb_info)) return 1;
      GBufferHost host(gb_info.n_pixels, gb_info.n_layers);
      const grt_gbuffer_arrays arr = host.arrays();
      if (grt_gbuffer_download(gbs[k], &arr) || grt_gbuffer_write_file(name.c_str(), &gb_info, &arr) ||
          (seq_adaptive && save_sub_sidecar(gbs[k], gb_info, name + ".sub"))) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      layers += gb_info.n_layers;
      if (seq_adaptive)
        std::fprintf(stderr, "[grt] sub-sample set: %llu selected pixels traced, saved to %s.sub\n",
                     (unsigned long long)per_frame[4 * k + 2], name.c_str());
      std::fprintf(stderr, "[grt] INFO saved g-buffer to %s\n", name.c_str());
    }
    if (seq_adaptive)
      std::fprintf(stderr, "[grt] sub-sample sets: %llu selected pixels of %u frames traced in one stacked top-up "
                   "(%llu sub-rays, %.1f ms)\n", (unsigned long long)srep.n_traced, K,
                   (unsigned long long)srep.top_up.rays, srep.trace_ms);
    ph_write = ms_since(t_phase);
    std::fprintf(stderr, "[grt] %llu rays, %llu accepted steps, %llu attempts, kernel %.1f ms; g-buffers: %llu layers, "
                 "scan + fill + split %.2f ms\n", (unsigned long long)st.rays, (unsigned long long)st.accepted_steps,
                 (unsigned long long)st.attempts, st.kernel_ms, layers, rep.fill_ms);
    std::fprintf(stderr, "[grt] sequence: %u frames in %u stacked launch(es) of up to %u, %u trace(s)\n", rep.n_frames,
                 rep.n_launches, rep.frames_per_launch, rep.n_traces);
    std::fprintf(stderr, "[grt] phases (ms): load %.1f, create %.1f, hip init %.1f, render %.1f, output %.1f, "
                 "write %.1f, since start %.1f\n", ph_load, ph_create, ph_init, ph_render, ph_output, ph_write,
                 ms_since(t_start));
    elapsed();
    for (grt_gbuffer* g : gbs) grt_gbuffer_destroy(g);
    grt_scene_destroy(scene);
    grt_host_scene_destroy(hs);
    return 0;
  }
  if (action == "reshade-sequence") {  // K traced frames under this config's appearance, shaded stacked
    const uint32_t K = (uint32_t)n_frames, w = (uint32_t)opts.width, h = (uint32_t)opts.height;
    const size_t n = (size_t)w * h;
    std::vector<grt_gbuffer*> gbs(K, nullptr);
    unsigned long long layers = 0;
    t_phase = clk::now();
    for (uint32_t k = 0; k < K; ++k) {
      std::string name;
      (void)expand_pattern(gbuffer_pattern, first_index + k, &name);
      if (grt_gbuffer_read_file(name.c_str(), &gb_info, nullptr)) {  // the sizes (checked before the load)
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      GBufferHost host(gb_info.n_pixels, gb_info.n_layers);
      const grt_gbuffer_arrays arr = host.arrays();
      if (grt_gbuffer_read_file(name.c_str(), &gb_info, &arr) || grt_gbuffer_upload(&gb_info, &arr, device, &gbs[k])) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      layers += gb_info.n_layers;
    }
    std::vector<double> xyza(n * 4 * K);
    grt_frame_out fo{nullptr, xyza.data(), nullptr, nullptr, nullptr, nullptr};
    float shade_ms = 0;
    // --adaptive-stacked: the adaptive frames, as `render` writes them
    grt_scene* tracer = nullptr;
    std::vector<uint8_t> status, stop;
    std::vector<uint32_t> steps;
    std::vector<uint64_t> nsel(K, 0), per_frame(4 * (size_t)K, 0);
    const uint64_t fail_cap = seq_adaptive ? 1u << 16 : 0;  // failed sub-rays logged per frame, as render-sequence
    std::vector<uint32_t> fail_pix(fail_cap * K), fail_sample(fail_cap * K), fail_steps(fail_cap * K);
    std::vector<uint8_t> fail_status(fail_cap * K), fail_stop(fail_cap * K);
    std::vector<grt_subsample_failures> fails(K);
    double mask[4];
    const double* maskp = nullptr;
    if (seq_adaptive) {
      // this config's scene with the files' recorded integration parameters (equal in every
      // file, checked above): it traces the sub-rays the sets do not hold yet, each with its
      // file's camera, and its appearance is the one applied
      grt_scene_desc td = *d;
      td.camera = gb_first.camera;
      td.max_steps = gb_first.max_steps;
      td.max_radius = gb_first.max_radius;
      td.step_size = gb_first.step_size;
      td.epsilon = gb_first.epsilon;
      td.horizon_epsilon = gb_first.horizon_epsilon;
      if (grt_scene_create(&td, &tracer)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      std::vector<uint64_t> before(K, 0);
      for (uint32_t k = 0; k < K; ++k) {  // the sidecars that exist
        std::string name;
        (void)expand_pattern(gbuffer_pattern, first_index + k, &name);
        const std::string sidecar = name + ".sub";
        FILE* f = std::fopen(sidecar.c_str(), "rb");
        if (!f) continue;
        std::fclose(f);
        grt_gbuffer_sub_info sub;
        if (grt_gbuffer_info_get(gbs[k], &gb_info) ||
            grt_gbuffer_sub_read_file(sidecar.c_str(), &gb_info, &sub, nullptr, nullptr)) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        GBufferSubHost sh(sub);
        const grt_gbuffer_arrays sarr = sh.rays.arrays();
        if (grt_gbuffer_sub_read_file(sidecar.c_str(), &gb_info, &sub, sh.sub_pixel.data(), &sarr) ||
            grt_gbuffer_sub_upload(gbs[k], &sub, sh.sub_pixel.data(), &sarr)) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        before[k] = sub.n_sub_pixels;
      }
      if (opts.show_sampling_mask) {
        grt_srgb_to_xyza(opts.sampling_mask_color[0], opts.sampling_mask_color[1], opts.sampling_mask_color[2], 255, mask);
        maskp = mask;
      }
      status.resize(n * K);
      stop.resize(n * K);
      steps.resize(n * K);
      for (uint32_t k = 0; k < K; ++k)
        fails[k] = grt_subsample_failures{fail_cap, fail_pix.data() + fail_cap * k, fail_sample.data() + fail_cap * k,
                                          fail_status.data() + fail_cap * k, 0, fail_stop.data() + fail_cap * k,
                                          fail_steps.data() + fail_cap * k};
      fo.status = status.data();
      fo.stop = stop.data();
      fo.steps = steps.data();
      grt_gbuffer_section_sequence_report srep;
      if (grt_gbuffer_shade_section_sequence(tracer, K, gbs.data(), &ac, maskp, tracer, &fo, nsel.data(), fails.data(),
                                             per_frame.data(), &srep)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      shade_ms = (float)srep.shade_ms;
      for (uint32_t k = 0; k < K; ++k)
        std::fprintf(stderr, "[grt] adaptive re-shade, frame %u: %llu selected pixels, %llu held, %llu traced\n", k,
                     (unsigned long long)per_frame[4 * k], (unsigned long long)per_frame[4 * k + 1],
                     (unsigned long long)per_frame[4 * k + 2]);
      std::fprintf(stderr, "[grt] adaptive re-shade: %llu selected pixels, %llu held, %llu traced in one stacked top-up "
                   "(%llu sub-rays, %.1f ms)\n", (unsigned long long)srep.n_selected, (unsigned long long)srep.n_held,
                   (unsigned long long)srep.n_traced, (unsigned long long)srep.top_up.rays, srep.trace_ms);
      for (uint32_t k = 0; k < K; ++k) {  // the sets that grew: the next re-shade finds them
        grt_gbuffer_sub_info after;
        if (grt_gbuffer_sub_info_get(gbs[k], &after)) return 1;
        if (after.n_sub_pixels <= before[k]) continue;
        std::string name;
        (void)expand_pattern(gbuffer_pattern, first_index + k, &name);
        if (grt_gbuffer_info_get(gbs[k], &gb_info) || save_sub_sidecar(gbs[k], gb_info, name + ".sub")) {
          std::fprintf(stderr, "Error: %s\n", grt_last_error());
          return 1;
        }
        std::fprintf(stderr, "[grt] INFO saved sub-sample set to %s.sub\n", name.c_str());
      }
    } else if (grt_gbuffer_shade_sequence(scene, K, gbs.data(), &fo, &shade_ms)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    ph_render = ms_since(t_phase);
    std::fprintf(stderr, "[grt] re-shaded %u frames of %llu pixels, %llu layers, kernel %.2f ms\n", K,
                 (unsigned long long)n, layers, shade_ms);
    for (uint32_t k = 0; k < K; ++k) {  // each frame tone-mapped on its own, as `reshade` does
      std::string name, raw;
      (void)expand_pattern(filename_pattern, first_index + k, &name);
      if (!raw_out.empty()) (void)expand_pattern(raw_out, first_index + k, &raw);
      const bool hdr = name.size() >= 4 && name.compare(name.size() - 4, 4, ".hdr") == 0;
      if (hdr) {
        std::fprintf(stderr, "[grt] INFO Creating HDR image\n");
      } else {
        std::fprintf(stderr, "[grt] INFO Creating non-HDR image\n");
        std::fprintf(stderr, "[grt] INFO Tone mapping method: %s\n",
                     opts.tone_mapping == GRT_TONE_GLOBAL_LINEAR ? "GlobalLinear" : "Reinhard");
      }
      if (seq_adaptive) {  // the frame's ray log, as `reshade --adaptive` writes it
        const std::vector<uint8_t> f_status(status.begin() + n * k, status.begin() + n * (k + 1));
        const std::vector<uint8_t> f_stop(stop.begin() + n * k, stop.begin() + n * (k + 1));
        const std::vector<uint32_t> f_steps(steps.begin() + n * k, steps.begin() + n * (k + 1));
        log_frame_rays(0, 0, w, f_status, f_stop, f_steps, ac.enabled && !maskp, nsel[k], fails[k]);
      }
      const std::vector<double> f_xyza(xyza.begin() + n * 4 * k, xyza.begin() + n * 4 * (k + 1));
      if (int wrc = write_frame(name, raw, f_xyza, w, h, opts.tone_mapping, device, &ph_output, &ph_write)) return wrc;
      std::fprintf(stderr, "[grt] INFO saved image to %s\n", name.c_str());
    }
    std::fprintf(stderr, "[grt] phases (ms): load %.1f, create %.1f, hip init %.1f, render %.1f, output %.1f, "
                 "write %.1f, since start %.1f\n", ph_load, ph_create, ph_init, ph_render, ph_output, ph_write,
                 ms_since(t_start));
    elapsed();
    for (grt_gbuffer* g : gbs) grt_gbuffer_destroy(g);
    if (tracer) grt_scene_destroy(tracer);
    grt_scene_destroy(scene);
    grt_host_scene_destroy(hs);
    return 0;
  }
  if (action == "render-sequence") {
    const uint32_t K = (uint32_t)path_cams.size(), w = (uint32_t)opts.width, h = (uint32_t)opts.height;
    const size_t n = (size_t)w * h;
    std::vector<grt_camera_desc> cams(K);
    for (uint32_t k = 0; k < K; ++k) {
      const std::vector<double>& c = path_cams[k];
      if (grt_host_scene_camera(hs, c.data(), c[3], c[4], c[5], &cams[k])) {
        std::fprintf(stderr, "Error: camera %u of %s: %s\n", k, camera_path.c_str(), grt_last_error());
        return 1;
      }
    }
    double mask[4];
    const double* maskp = nullptr;
    if (opts.show_sampling_mask) {
      grt_srgb_to_xyza(opts.sampling_mask_color[0], opts.sampling_mask_color[1], opts.sampling_mask_color[2], 255, mask);
      maskp = mask;
    }
    const bool supersampled = ac.enabled || maskp;
    std::vector<double> xyza(n * 4 * K);
    std::vector<uint8_t> status(n * K), stop(n * K);
    std::vector<uint32_t> steps(n * K);
    // failed supersample sub-rays (raytracer.rs:357-362), up to 64K logged per frame
    const uint64_t fail_cap = supersampled && !maskp ? 1u << 16 : 0;
    std::vector<uint32_t> fail_pix(fail_cap * K), fail_sample(fail_cap * K), fail_steps(fail_cap * K);
    std::vector<uint8_t> fail_status(fail_cap * K), fail_stop(fail_cap * K);
    std::vector<grt_subsample_failures> fails(K);
    for (uint32_t k = 0; k < K; ++k)
      fails[k] = grt_subsample_failures{fail_cap, fail_pix.data() + fail_cap * k, fail_sample.data() + fail_cap * k,
                                        fail_status.data() + fail_cap * k, 0, fail_stop.data() + fail_cap * k,
                                        fail_steps.data() + fail_cap * k};
    std::vector<uint64_t> nsel(K, 0);
    grt_frame_out fo{nullptr, xyza.data(), nullptr, status.data(), stop.data(), steps.data()};
    grt_stats st;
    grt_sequence_report rep;
    t_phase = clk::now();
    if (grt_render_sequence(scene, device, K, cams.data(), &ac, maskp, &fo, nsel.data(), &st, fails.data(), &rep)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
    ph_render = ms_since(t_phase);
    for (uint32_t k = 0; k < K; ++k) {  // each frame: the lines and the output of `render`
      std::string name, raw;
      (void)expand_pattern(filename_pattern, first_index + k, &name);
      if (!raw_out.empty()) (void)expand_pattern(raw_out, first_index + k, &raw);
      const bool hdr = name.size() >= 4 && name.compare(name.size() - 4, 4, ".hdr") == 0;
      if (hdr) {  // raytracer.rs:468-469, :481-483
        std::fprintf(stderr, "[grt] INFO Creating HDR image\n");
      } else {
        std::fprintf(stderr, "[grt] INFO Creating non-HDR image\n");
        std::fprintf(stderr, "[grt] INFO Tone mapping method: %s\n",
                     opts.tone_mapping == GRT_TONE_GLOBAL_LINEAR ? "GlobalLinear" : "Reinhard");
      }
      if (supersampled)  // raytracer.rs:264-267
        std::fprintf(stderr, "[grt] INFO Rendering section from (%u, %u) to (%u, %u) with supersampling\n", 0u, 0u, h, w);
      const std::vector<uint8_t> f_status(status.begin() + n * k, status.begin() + n * (k + 1));
      const std::vector<uint8_t> f_stop(stop.begin() + n * k, stop.begin() + n * (k + 1));
      const std::vector<uint32_t> f_steps(steps.begin() + n * k, steps.begin() + n * (k + 1));
      log_frame_rays(0, 0, w, f_status, f_stop, f_steps, supersampled && !maskp, nsel[k], fails[k]);
      if (supersampled)  // raytracer.rs:313-316
        std::fprintf(stderr, "[grt] INFO Finished rendering section from (%u, %u) to (%u, %u)\n", 0u, 0u, h, w);
      const std::vector<double> f_xyza(xyza.begin() + n * 4 * k, xyza.begin() + n * 4 * (k + 1));
      if (int wrc = write_frame(name, raw, f_xyza, w, h, opts.tone_mapping, device, &ph_output, &ph_write)) return wrc;
      std::fprintf(stderr, "[grt] INFO saved image to %s\n", name.c_str());  // raytracer.rs:494
    }
    unsigned long long nsel_all = 0;
    for (uint64_t v : nsel) nsel_all += v;
    std::fprintf(stderr, "[grt] %llu rays, %llu accepted steps, %llu attempts, %llu supersampled pixels, kernel %.1f ms "
                 "(%.3e steps/s)\n",
                 (unsigned long long)st.rays, (unsigned long long)st.accepted_steps, (unsigned long long)st.attempts,
                 nsel_all, st.kernel_ms, st.accepted_steps / (st.kernel_ms * 1e-3));
    std::fprintf(stderr, "[grt] sequence: %u frames in %u stacked launch(es) of up to %u; trace %.1f ms, supersample "
                 "%.1f ms\n", rep.n_frames, rep.n_launches, rep.frames_per_launch, rep.trace_ms, rep.supersample_ms);
    std::fprintf(stderr, "[grt] phases (ms): load %.1f, create %.1f, hip init %.1f, render %.1f, output %.1f, "
                 "write %.1f, since start %.1f\n", ph_load, ph_create, ph_init, ph_render, ph_output, ph_write,
                 ms_since(t_start));
    elapsed();
    grt_scene_destroy(scene);
    grt_host_scene_destroy(hs);
    return 0;
  }
  if (action != "render") {
    int rc;
    if (action == "render-ray") {  // Raytracer::integrate_ray_at_point (raytracer.rs:499-507)
      const double row = (double)ray_row, col = (double)ray_col;
      rc = trace_and_save(scene, device, d, true, &row, &col, filename);
    } else {
      if (ray_position.size() != 3) {
        std::fprintf(stderr, "Error: Position must be a vector of length 3, got %zu values\n", ray_position.size());
        return 1;
      }
      if (ray_direction.size() != 3) {
        std::fprintf(stderr, "Error: Direction must be a vector of length 3, got %zu values\n", ray_direction.size());
        return 1;
      }
      double pos[4], mom[4];
      if (grt_ray_at(d->geometry, d->radius, d->a, ray_position.data(), ray_direction.data(), pos, mom)) {
        std::fprintf(stderr, "Error: %s\n", grt_last_error());
        return 1;
      }
      rc = trace_and_save(scene, device, d, false, pos, mom, filename);
    }
    grt_scene_destroy(scene);
    grt_host_scene_destroy(hs);
    if (rc == 0) elapsed();
    return rc;
  }
  uint32_t r0 = from_row < 0 ? 0 : (uint32_t)from_row, c0 = from_col < 0 ? 0 : (uint32_t)from_col;
  uint32_t r1 = to_row < 0 ? (uint32_t)opts.height : (uint32_t)to_row;
  uint32_t c1 = to_col < 0 ? (uint32_t)opts.width : (uint32_t)to_col;
  uint32_t w = c1 - c0, h = r1 - r0;
  std::vector<double> xyza((size_t)w * h * 4);
  double mask[4];
  const double* maskp = nullptr;
  if (opts.show_sampling_mask) {
    grt_srgb_to_xyza(opts.sampling_mask_color[0], opts.sampling_mask_color[1], opts.sampling_mask_color[2], 255, mask);
    maskp = mask;
  }
  grt_stats st;
  uint64_t nsel = 0;
  std::vector<uint8_t> status((size_t)w * h);
  // failed supersample sub-rays (raytracer.rs:357-362), up to 1M logged
  const uint64_t fail_cap = 1u << 20;
  std::vector<uint32_t> fail_pix(fail_cap), fail_sample(fail_cap);
  std::vector<uint8_t> fail_status(fail_cap), fail_stop(fail_cap);
  std::vector<uint32_t> fail_steps(fail_cap);
  grt_subsample_failures fails{fail_cap, fail_pix.data(), fail_sample.data(), fail_status.data(), 0,
                               fail_stop.data(), fail_steps.data()};
  std::vector<uint8_t> stop((size_t)w * h);
  std::vector<uint32_t> steps((size_t)w * h);
  const bool supersampled = ac.enabled || maskp;
  const bool hdr = filename.size() >= 4 && filename.compare(filename.size() - 4, 4, ".hdr") == 0;
  if (hdr) {  // raytracer.rs:468-469, :481-483
    std::fprintf(stderr, "[grt] INFO Creating HDR image\n");
  } else {
    std::fprintf(stderr, "[grt] INFO Creating non-HDR image\n");
    std::fprintf(stderr, "[grt] INFO Tone mapping method: %s\n",
                 opts.tone_mapping == GRT_TONE_GLOBAL_LINEAR ? "GlobalLinear" : "Reinhard");
  }
  const bool multi = !multi_devices.empty();
  if (supersampled)  // raytracer.rs:264-267
    std::fprintf(stderr, "[grt] INFO Rendering section from (%u, %u) to (%u, %u) with supersampling\n", r0, c0, r1,
                 c1);
  t_phase = clk::now();
  grt_multi_report mrep;
  if (multi) {
    // the frame over several GPUs: cyclic row bands, one host thread per device, one RCCL
    // gather of f64 XYZA + class + status + stop + steps (39 B per pixel) to the first
    grt_frame_out fo{nullptr, xyza.data(), nullptr, status.data(), stop.data(), steps.data()};
    if (grt_render_frame_multi(scene, (int)multi_devices.size(), multi_devices.data(), band_rows, &ac, maskp, &fo,
                               &nsel, &st, &fails, &mrep)) {
      std::fprintf(stderr, "Error: %s\n", grt_last_error());
      return 1;
    }
  } else if (grt_render_section_ex(scene, device, r0, c0, r1, c1, &ac, maskp, xyza.data(), nullptr, &nsel, &st,
                                   status.data(), &fails, stop.data(), steps.data())) {
    std::fprintf(stderr, "Error: %s\n", grt_last_error());
    return 1;
  }
  ph_render = ms_since(t_phase);
  log_frame_rays(r0, c0, w, status, stop, steps, supersampled && !maskp, nsel, fails);
  if (supersampled)  // raytracer.rs:313-316
    std::fprintf(stderr, "[grt] INFO Finished rendering section from (%u, %u) to (%u, %u)\n", r0, c0, r1, c1);
  std::fprintf(stderr, "[grt] %llu rays, %llu accepted steps, %llu attempts, %llu supersampled pixels, kernel %.1f ms "
               "(%.3e steps/s)\n",
               (unsigned long long)st.rays, (unsigned long long)st.accepted_steps, (unsigned long long)st.attempts,
               (unsigned long long)nsel, st.kernel_ms, st.accepted_steps / (st.kernel_ms * 1e-3));
  if (multi) {
    std::string per;
    for (uint32_t k = 0; k < mrep.n_devices; ++k) {
      char b[96];
      std::snprintf(b, sizeof(b), "%s%d: %llu rows %.1f ms", k ? ", " : "", multi_devices[k],
                    (unsigned long long)mrep.rows[k], mrep.trace_ms[k]);
      per += b;
    }
    std::fprintf(stderr, "[grt] %u GPU(s) [%s]; transport %s, allgather %.2f ms, gather %.2f ms (%u B per pixel), "
                 "%u trace(s)\n", mrep.n_devices, per.c_str(), transport_name(mrep.transport), mrep.allgather_ms,
                 mrep.gather_ms, mrep.record_bytes, mrep.attempts);
  }
  if (st.march_jobs)
    std::fprintf(stderr, "[grt] VolumetricDisc: %llu raymarches, %llu samples (%llu with noise, %llu emitting)\n",
                 (unsigned long long)st.march_jobs, (unsigned long long)st.march_samples,
                 (unsigned long long)st.march_noise_samples, (unsigned long long)st.march_emit_samples);
  if (int wrc = write_frame(filename, raw_out, xyza, w, h, opts.tone_mapping, multi ? multi_devices[0] : device,
                            &ph_output, &ph_write))
    return wrc;
  std::fprintf(stderr, "[grt] INFO saved image to %s\n", filename.c_str());  // raytracer.rs:494
  // where the wall time went: TOML + texture decode + LUTs; the descriptor copy; the render
  // call (device upload on first use, trace, supersampling, D2H); tone map; encode + write
  std::fprintf(stderr, "[grt] phases (ms): load %.1f, create %.1f, hip init %.1f, render %.1f, output %.1f, "
               "write %.1f, since start %.1f%s%s\n", ph_load, ph_create, ph_init, ph_render, ph_output, ph_write,
               ms_since(t_start), multi ? "; transport " : "", multi ? transport_name(mrep.transport) : "");
  elapsed();
  // teardown after the reference's measured span (main.rs:175-176 logs before its drops;
  // the multi-GPU set-up is released by hip_init_join)
  grt_scene_destroy(scene);
  grt_host_scene_destroy(hs);
  return 0;
}
