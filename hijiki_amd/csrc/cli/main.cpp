// hijiki-hip — command line of the reference (`struct Opt` / `main`, src/main.rs:1426-1494) on the MI355X path:
//
//   hijiki-hip [--put-cbox-spheres] [--use-bvh] [-w/--width 800] [-h/--height 600] [--present-interval 128]
//              [-s/--sample-count 64] [-o/--output-image /tmp/output.exr] [--seed 1] [--textures] [--env FILE [--env-scale S]]
//              [--bake-lightmap WxH [--gutter 2] [--filter N[,sp[,sn[,sc]]]] [--adaptive min,step,max,rel[,floor]] [--sample-map FILE]]
//              [--aovs PREFIX [--aov-follow N]] [--denoise FILE [--denoise-params iters,sn,sz,sl,sa]] <scene.obj | synthetic:KIND>
//
// Same flags and defaults (including `-h` meaning height and brute-force traversal unless --use-bvh).  There is
// no preview window, so --present-interval is accepted and ignored; --seed replaces the OS-seeded block RNG; --textures (not
// upstream) renders the MTL's map_Kd images on diffuse materials; --env (not upstream) lights the scene with a lat-long HDR image;
// --bake-lightmap WxH (not upstream) writes no camera frame but the scene's light-map atlas: hj_bake_lightmap over all triangles at
// -s samples a texel, seed --seed, stride 1, offset 1e-3, --gutter dilation passes; the atlas's rgb goes to -o, row v = 0 on top.
// --filter N[,sp[,sn[,sc]]] (not upstream) runs N iterations of hj_filter_lightmap's edge-avoiding a-trous filter between the bake's
// scatter and its dilation (hj_bake_lightmap_filtered): sp, sn, sc are sigma_position (default: 1 % of the root box's diagonal),
// sigma_normal (0.5) and sigma_color (0: off) - a starting point, not a tuned optimum.
// --adaptive min,step,max,rel[,floor] (not upstream) bakes with hj_bake_lightmap_adaptive: every texel gets `min` samples, then `step`
// more a round up to `max`, until the standard error of its mean luminance is at most rel * max(mean, floor) (floor: 0.01 unless
// given); -s is then ignored, with a note on stderr.  --sample-map FILE writes the samples each texel received as a one-channel PFM.
// --aovs PREFIX (not upstream) writes, beside the frame, PREFIX_albedo.pfm, PREFIX_normal.pfm and PREFIX_depth.pfm (the depth in all
// three channels): hj_render_aovs_frame for the frame's own -s and --seed, its sums divided by the sample count (albedo) or the hit
// count (normal, depth), 0 where the count is 0.
// --aov-follow N (not upstream, with --aovs) follows mirror and glass through up to N specular surfaces: hj_render_aovs_frame_followed.
// --denoise FILE (not upstream) writes, beside the frame, the frame denoised: hj_render_aovs_frame for the frame's own -s and --seed,
// then hj_denoise_frame over the framebuffer on the device (beauty = NULL); the rgb goes to FILE through the writer its extension
// chooses.  --denoise-params iters,sn,sz,sl,sa: the iterations (5) and the sigmas of normal (0.5), depth (1), luminance (4) and
// albedo (0.1) - SVGF's starting points where it has them, guesses elsewhere, not tuned.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/hijiki_hip.h"
#include "../../../include/hijiki_host.h"
#include "../host/scene.hpp"

namespace {

struct Opt {
  bool put_cbox_spheres = false, use_bvh = false, device_bvh = false, textures = false;
  uint32_t width = 800, height = 600, present_interval = 128, sample_count = 64;
  uint64_t seed = 1;
  std::string output_image = "/tmp/output.exr", scene, env;
  float env_scale = 1.0f;
  uint32_t bake_w = 0, bake_h = 0, gutter = 2;             // --bake-lightmap WxH (0: render a frame), --gutter
  bool gutter_given = false;
  uint32_t filter_n = 0;                                   // --filter N[,sp[,sn[,sc]]]: iterations (0: none)
  float filter_sp = -1.0f, filter_sn = 0.5f, filter_sc = 0.0f;   // (sp < 0: 1 % of the root box's diagonal)
  bool filter_given = false;
  hj_adaptive_opts adaptive{0u, 0u, 0u, 0.0f, 0.01f};      // --adaptive min,step,max,rel[,floor]
  bool adaptive_given = false, samples_given = false;      // (samples_given: -s was on the command line)
  std::string sample_map;                                  // --sample-map FILE
  std::string aovs;                                        // --aovs PREFIX
  uint32_t aov_follow = 0;                                 // --aov-follow N: mirror and glass followed through N surfaces
  bool aov_follow_given = false;
  std::string denoise;                                     // --denoise FILE
  hj_denoise_opts denoise_opts{5u, 0.5f, 1.0f, 4.0f, 0.1f, 0u};   // --denoise-params iters,sn,sz,sl,sa
  bool denoise_params_given = false;
};

[[noreturn]] void usage(const char* msg) {
  if (msg) std::fprintf(stderr, "error: %s\n\n", msg);
  std::fprintf(stderr,
               "USAGE: hijiki-hip [FLAGS] [OPTIONS] <scene>\n\n"
               "FLAGS:\n    --put-cbox-spheres    Add a mirror and glass sphere to the scene\n"
               "    --use-bvh             Use a BVH to optimize intersections\n"
               "    --device-bvh          (not upstream) build the tree on the GPU (LBVH, stays there: fast start) instead of on the host (SAH)\n"
               "    --textures            (not upstream) diffuse materials with map_Kd take their colour from that image (PFM or P6 PPM)\n\n"
               "        --env <file>                             (not upstream) light the scene with this lat-long image (PFM or P6 PPM)\n"
               "        --env-scale <scale>                      [default: 1] (not upstream) radiance scale of --env\n"
               "        --bake-lightmap <W>x<H>                  (not upstream) bake the light-map atlas of the scene's UVs instead of a frame\n"
               "        --gutter <passes>                        [default: 2] (not upstream) dilation passes of --bake-lightmap, 0 ... 64\n"
               "        --filter <N>[,<sp>[,<sn>[,<sc>]]]        (not upstream) N = 0 ... 8 iterations of the edge-avoiding a-trous filter over the baked\n"
               "                                                 atlas; sigmas of position [default: 1 %% of the scene box's diagonal], normal [0.5]\n"
               "                                                 and colour [0 = off]: a starting point, not a tuned optimum\n"
               "        --adaptive <min>,<step>,<max>,<rel>[,<floor>]  (not upstream) --bake-lightmap with the sample count decided per texel:\n"
               "                                                 min samples, then step more a round up to max, until the standard error of the\n"
               "                                                 mean luminance is at most rel * max(mean, floor [0.01]); -s is ignored\n"
               "        --sample-map <file>                      (not upstream) with --adaptive: the samples per texel as a one-channel PFM\n"
               "        --aovs <prefix>                          (not upstream) beside the frame: <prefix>_albedo.pfm, <prefix>_normal.pfm and\n"
               "                                                 <prefix>_depth.pfm - the means over the frame's own primary rays of the first\n"
               "                                                 hit's albedo, shading normal and distance (0 where nothing was hit)\n"
               "        --aov-follow <n>                         (not upstream) with --aovs: mirror and glass are followed through up to n\n"
               "                                                 (0 ... 8) specular surfaces and show what they show [default: 0]\n"
               "        --denoise <file>                         (not upstream) beside the frame: the frame denoised by the AOV-guided a-trous\n"
               "                                                 filter (.exr, .pfm or .png)\n"
               "        --denoise-params <iters>,<sn>,<sz>,<sl>,<sa>  (not upstream) iterations 0 ... 8 [5] and the sigmas of normal [0.5], depth [1],\n"
               "                                                 luminance [4] and albedo [0.1] of --denoise: starting points, not tuned\n"
               "OPTIONS:\n    -h, --height <height>                        [default: 600]\n"
               "    -o, --output-image <output-image>            [default: /tmp/output.exr] (.exr, .pfm or .png)\n"
               "        --present-interval <present-interval>    [default: 128] (ignored: no preview window)\n"
               "    -s, --sample-count <sample-count>            [default: 64]\n"
               "        --seed <seed>                            [default: 1]\n"
               "    -w, --width <width>                          [default: 800]\n\n"
               "ARGS:\n    <scene>    The scene (OBJ file) to render, or synthetic:cbox | synthetic:spheres | synthetic:mesh\n");
  std::exit(msg ? 2 : 0);
}

Opt parse(int argc, char** argv) {
  Opt o;
  auto value = [&](int& i) -> std::string {
    if (i + 1 >= argc) usage((std::string("missing value for ") + argv[i]).c_str());
    return argv[++i];
  };
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--put-cbox-spheres") o.put_cbox_spheres = true;
    else if (a == "--use-bvh") o.use_bvh = true;
    else if (a == "--device-bvh") o.device_bvh = true;
    else if (a == "--textures") o.textures = true;
    else if (a == "-w" || a == "--width") o.width = (uint32_t)std::stoul(value(i));
    else if (a == "-h" || a == "--height") o.height = (uint32_t)std::stoul(value(i));
    else if (a == "--present-interval") o.present_interval = (uint32_t)std::stoul(value(i));
    else if (a == "-s" || a == "--sample-count") { o.sample_count = (uint32_t)std::stoul(value(i)); o.samples_given = true; }
    else if (a == "-o" || a == "--output-image") o.output_image = value(i);
    else if (a == "--seed") o.seed = std::stoull(value(i));
    else if (a == "--env") o.env = value(i);
    else if (a == "--env-scale") {
      const std::string v = value(i);
      char* end = nullptr;
      o.env_scale = std::strtof(v.c_str(), &end);
      if (end == v.c_str() || *end != '\0' || !(o.env_scale >= 0.0f) || o.env_scale > 3.0e38f) usage(("bad --env-scale " + v).c_str());
    }
    else if (a == "--bake-lightmap") {
      const std::string v = value(i);
      unsigned w = 0, h = 0;
      char tail = 0;
      if (std::sscanf(v.c_str(), "%ux%u%c", &w, &h, &tail) != 2 || w == 0 || h == 0 || w > 16384u || h > 16384u || (uint64_t)w * h > (1ull << 26))
        usage(("bad --bake-lightmap " + v + " (WxH, 1 ... 16384 each, at most 2^26 texels)").c_str());
      o.bake_w = w; o.bake_h = h;
    }
    else if (a == "--gutter") {
      const unsigned long g = std::stoul(value(i));
      if (g > HJ_LIGHTMAP_MAX_GUTTER) usage("--gutter above 64");
      o.gutter = (uint32_t)g;
      o.gutter_given = true;
    }
    else if (a == "--filter") {
      const std::string v = value(i);
      unsigned n = 0;
      float sg[3] = {-1.0f, 0.5f, 0.0f};
      char tail = 0;
      const int got = std::sscanf(v.c_str(), "%u,%f,%f,%f%c", &n, &sg[0], &sg[1], &sg[2], &tail);
      bool ok = got >= 1 && got <= 4 && n <= HJ_LIGHTMAP_FILTER_MAX_ITERATIONS && v.find_first_not_of("0123456789.,eE+-") == std::string::npos && v.back() != ',';
      for (int k = 0; ok && k < got - 1; k++) ok = sg[k] >= 0.0f && sg[k] <= 3.0e38f;
      if (!ok) usage(("bad --filter " + v + " (N[,sp[,sn[,sc]]]: N = 0 ... 8, sigmas finite and >= 0)").c_str());
      o.filter_n = n; o.filter_sp = sg[0]; o.filter_sn = sg[1]; o.filter_sc = sg[2];
      o.filter_given = true;
    }
    else if (a == "--adaptive") {
      const std::string v = value(i);
      unsigned mn = 0, stp = 0, mx = 0;
      float rel = 0.0f, fl = 0.01f;
      char tail = 0;
      const int got = std::sscanf(v.c_str(), "%u,%u,%u,%f,%f%c", &mn, &stp, &mx, &rel, &fl, &tail);
      const bool ok = (got == 4 || got == 5) && v.find_first_not_of("0123456789.,eE+-") == std::string::npos && v.back() != ',' && mn >= 2 && stp >= 1 &&
                      mx >= mn && mx <= 65536u && 1u + (mx - mn + stp - 1u) / stp <= 64u && rel >= 0.0f && rel <= 3.0e38f && fl >= 0.0f && fl <= 3.0e38f;
      if (!ok)
        usage(("bad --adaptive " + v + " (min,step,max,rel[,floor]: 2 <= min <= max <= 65536, step >= 1, at most 64 rounds, rel and floor finite and >= 0)").c_str());
      o.adaptive = hj_adaptive_opts{mn, stp, mx, rel, fl};
      o.adaptive_given = true;
    }
    else if (a == "--sample-map") o.sample_map = value(i);
    else if (a == "--aovs") o.aovs = value(i);
    else if (a == "--aov-follow") {
      const std::string v = value(i);
      unsigned n = 0;
      char tail = 0;
      if (std::sscanf(v.c_str(), "%u%c", &n, &tail) != 1 || v.find_first_not_of("0123456789") != std::string::npos || n > HJ_AOV_MAX_FOLLOW)
        usage(("bad --aov-follow " + v + " (0 ... 8)").c_str());
      o.aov_follow = n;
      o.aov_follow_given = true;
    }
    else if (a == "--denoise") o.denoise = value(i);
    else if (a == "--denoise-params") {
      const std::string v = value(i);
      unsigned n = 0;
      float sg[4] = {0.0f, 0.0f, 0.0f, 0.0f};
      char tail = 0;
      const int got = std::sscanf(v.c_str(), "%u,%f,%f,%f,%f%c", &n, &sg[0], &sg[1], &sg[2], &sg[3], &tail);
      bool ok = got == 5 && n <= HJ_DENOISE_MAX_ITERATIONS && v.find_first_not_of("0123456789.,eE+-") == std::string::npos;
      for (int k = 0; ok && k < 4; k++) ok = sg[k] >= 0.0f && sg[k] <= 3.0e38f;
      if (!ok) usage(("bad --denoise-params " + v + " (iters,sn,sz,sl,sa: iters = 0 ... 8, sigmas finite and >= 0)").c_str());
      o.denoise_opts = hj_denoise_opts{n, sg[0], sg[1], sg[2], sg[3], 0u};
      o.denoise_params_given = true;
    }
    else if (a == "--help") usage(nullptr);
    else if (!a.empty() && a[0] == '-') usage(("unknown flag " + a).c_str());
    else if (o.scene.empty()) o.scene = a;
    else usage("more than one scene given");
  }
  if (o.scene.empty()) usage("the <scene> argument is required");
  if (o.env.empty() && o.env_scale != 1.0f) usage("--env-scale without --env");
  if (o.gutter_given && o.bake_w == 0) usage("--gutter without --bake-lightmap");
  if (o.filter_given && o.bake_w == 0) usage("--filter without --bake-lightmap");
  if (o.adaptive_given && o.bake_w == 0) usage("--adaptive without --bake-lightmap");
  if (!o.sample_map.empty() && !o.adaptive_given) usage("--sample-map without --adaptive");
  if (!o.aovs.empty() && o.bake_w != 0) usage("--aovs belongs to a frame, not to --bake-lightmap");
  if (o.aov_follow_given && o.aovs.empty()) usage("--aov-follow without --aovs");
  if (!o.denoise.empty() && o.bake_w != 0) usage("--denoise belongs to a frame, not to --bake-lightmap");
  if (o.denoise_params_given && o.denoise.empty()) usage("--denoise-params without --denoise");
  if (o.adaptive_given && o.samples_given) std::fprintf(stderr, "note: --adaptive decides the samples per texel; -s %u is ignored\n", o.sample_count);
  if (o.filter_given && o.filter_sp < 0.0f && o.device_bvh) usage("--filter with --device-bvh needs its sigma_position (no root box on the host)");
  return o;
}

// the sample map as a one-channel PFM ("Pf"): the counts as floats (exact: at most 65536), bottom row first on disk
void write_grey_pfm(const std::string& path, uint32_t w, uint32_t h, const std::vector<uint32_t>& words) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot create " + path);
  std::fprintf(f, "Pf\n%u %u\n-1.0\n", w, h);
  std::vector<float> row(w);
  for (uint32_t y = 0; y < h; y++) {
    for (uint32_t x = 0; x < w; x++) row[x] = (float)words[(size_t)(h - 1 - y) * w + x];
    std::fwrite(row.data(), sizeof(float), w, f);
  }
  if (std::fclose(f) != 0) throw std::runtime_error("write failed: " + path);
}

void check(hj_context* ctx, int rc, const char* what) {
  if (rc != HJ_OK) throw std::runtime_error(std::string(what) + ": " + hj_last_error(ctx));
}

}  // namespace

int main(int argc, char** argv) {
  try {
    const Opt opt = parse(argc, argv);
    hijiki::Scene scene;
    if (opt.scene.rfind("synthetic:", 0) == 0) {
      const std::string kind = opt.scene.substr(10);
      scene = hijiki::make_synthetic(kind == "spheres" ? HJH_SYNTH_CBOX_SPHERES : kind == "mesh" ? HJH_SYNTH_CBOX_MESH : HJH_SYNTH_CBOX,
                                     kind == "mesh" ? 1000000u : 0u, 1);
    } else {
      scene = hijiki::scene_from_obj(opt.scene, opt.textures);         // Scene::from_obj, src/main.rs:1462
    }
    if (opt.put_cbox_spheres) hijiki::put_cbox_spheres(scene);         // src/main.rs:1463-1483
    uint32_t env_tex = 0;
    if (!opt.env.empty()) {                                            // --env: the image joins the scene's textures, bilinear
      uint32_t w = 0, h = 0;
      std::vector<float> rgba;
      hijiki::read_texture_image(opt.env, w, h, rgba);
      env_tex = hijiki::add_texture(scene, w, h, rgba.data(), 4, HJ_TEX_BILINEAR);
    }
    std::printf("Building BVH\n");                                     // src/main.rs:198
    // --device-bvh: the fast start - no tree on the host at all; hj_build_bvh_device leaves its tree on the device and
    // hj_scene_upload (scene->bvh == NULL) takes it over there: a 1 M-triangle scene is renderable 40 ms after its shapes exist
    hijiki::CompiledScene cs = hijiki::compile(scene, !opt.device_bvh);  // src/main.rs:1486
    hj_context* ctx = nullptr;
    if (hj_context_create(0, &ctx) != HJ_OK) throw std::runtime_error(hj_last_error(nullptr));
    size_t num_nodes = cs.bvh.size();
    const hj_scene_desc desc = cs.desc();                              // (bvh == NULL, num_bvh_nodes == 0 on the device route)
    if (opt.device_bvh) check(ctx, hj_build_bvh_device(ctx, &desc, nullptr, 0, &num_nodes), "device BVH build");
    std::printf("Built BVH with %zu nodes\n", num_nodes);              // src/main.rs:200

    const hj_texture_set tex = cs.texture_set();
    if (!opt.env.empty()) {
      // the environment's share of next-event samples: all of them without emitters, none for a black image, half otherwise
      hj_environment env{env_tex, {opt.env_scale, opt.env_scale, opt.env_scale}, 1.0f, 0u};
      double weight = 0.0;
      check(nullptr, hj_debug_env_distribution(&tex, &env, nullptr, nullptr, nullptr, nullptr, &weight), "environment");
      if (desc.num_emitters != 0) env.select_prob = weight > 0.0 ? 0.5f : 0.0f;
      check(ctx, hj_scene_upload_env(ctx, &desc, &tex, &env), "scene upload");
    } else {
      check(ctx, opt.textures ? hj_scene_upload_textured(ctx, &desc, &tex) : hj_scene_upload(ctx, &desc), "scene upload");
    }
    const auto save_to = [](const std::string& path, uint32_t w, uint32_t h, const float* rgb) {
      const std::string ext = path.size() > 4 ? path.substr(path.size() - 4) : "";
      if (ext == ".pfm") hijiki::write_pfm(path, w, h, rgb);
      else if (ext == ".png") hijiki::write_png(path, w, h, rgb);   // the preview image
      else hijiki::write_exr(path, w, h, rgb);
    };
    const auto save = [&](uint32_t w, uint32_t h, const float* rgb) { save_to(opt.output_image, w, h, rgb); };
    if (opt.bake_w != 0) {                                             // --bake-lightmap: the atlas instead of a frame
      const hj_lightmap_desc lm{opt.bake_w, opt.bake_h, 0u, 0u, (uint32_t)opt.seed, 1u, 1e-3f, 0u};
      std::vector<float> rgba((size_t)opt.bake_w * opt.bake_h * 4), rgb((size_t)opt.bake_w * opt.bake_h * 3);
      size_t texels = 0;
      hj_render_stats bst;
      std::printf("Baking %u x %u texels...\n", opt.bake_w, opt.bake_h);
      hj_lightmap_filter flt{0u, 0.0f, 0.0f, 0.0f, 0u};
      if (opt.filter_given) {
        float sp = opt.filter_sp;
        if (sp < 0.0f) {                                                 // 1 % of the root box's diagonal
          const hj_bvh_node& root = cs.bvh.at(0);
          const float dx = root.aabb_max[0] - root.aabb_min[0], dy = root.aabb_max[1] - root.aabb_min[1], dz = root.aabb_max[2] - root.aabb_min[2];
          sp = 0.01f * std::sqrt((dx * dx + dy * dy) + dz * dz);
        }
        flt = hj_lightmap_filter{opt.filter_n, sp, opt.filter_sn, opt.filter_sc, 0u};
        std::printf("Filter: %u iterations, sigmas %g (position), %g (normal), %g (colour)\n", flt.iterations, (double)sp, (double)flt.sigma_normal,
                    (double)flt.sigma_color);
      }
      if (opt.adaptive_given) {
        std::vector<uint32_t> smap(opt.sample_map.empty() ? 0 : (size_t)opt.bake_w * opt.bake_h);
        std::printf("Adaptive: %u samples, then %u a round up to %u; rel_error %g, floor %g\n", opt.adaptive.spp_min, opt.adaptive.spp_step, opt.adaptive.spp_max,
                    (double)opt.adaptive.rel_error, (double)opt.adaptive.floor);
        check(ctx, hj_bake_lightmap_adaptive(ctx, &lm, &opt.adaptive, opt.gutter, opt.filter_given ? &flt : nullptr, nullptr, rgba.data(),
                                             smap.empty() ? nullptr : smap.data(), &texels, &bst), "bake");
        std::printf("Adaptive rounds: %llu\n", (unsigned long long)bst.bounce_rounds);
        if (!smap.empty()) write_grey_pfm(opt.sample_map, opt.bake_w, opt.bake_h, smap);
      } else if (opt.filter_given) {
        check(ctx, hj_bake_lightmap_filtered(ctx, &lm, opt.sample_count, opt.gutter, &flt, nullptr, rgba.data(), &texels, &bst), "bake");
      } else {
        check(ctx, hj_bake_lightmap(ctx, &lm, opt.sample_count, opt.gutter, nullptr, rgba.data(), &texels, &bst), "bake");
      }
      std::printf("Gathered %llu paths at %zu texels in %.6fs\n", (unsigned long long)bst.paths, texels, bst.total_ms * 1e-3);
      for (size_t t = 0; t < (size_t)opt.bake_w * opt.bake_h; t++)
        for (int c = 0; c < 3; c++) rgb[3 * t + c] = rgba[4 * t + c];
      save(opt.bake_w, opt.bake_h, rgb.data());
      hj_context_destroy(ctx);
      return 0;
    }
    check(ctx, hj_framebuffer_create(ctx, opt.width, opt.height, nullptr), "framebuffer");
    hj_render_opts ro;
    hj_default_render_opts(&ro);
    ro.use_bvh = opt.use_bvh ? 1u : 0u;                                // --use-bvh, src/main.rs:1432-1434
    hj_render_stats st;
    // the window title of the preview shows the percentage, updated every --present-interval blocks (src/main.rs:1335-1340)
    hj_set_progress_callback(ctx, [](void*, uint64_t done, uint64_t total) {
      std::fprintf(stderr, "\r%3.3f%% %llu/%llu", 100.0 * (double)done / (double)(total ? total : 1),      // the title's format
                   (unsigned long long)done, (unsigned long long)total);
      if (done >= total) std::fprintf(stderr, "\n");
    }, nullptr, opt.present_interval);
    {   // resource creation belongs to Renderer::new (src/main.rs:1167-1314), not to the timed render
      const uint64_t per_pass = (uint64_t)((opt.width + HJ_BLOCK_SIZE - 1) / HJ_BLOCK_SIZE) * ((opt.height + HJ_BLOCK_SIZE - 1) / HJ_BLOCK_SIZE);
      check(ctx, hj_reserve(ctx, (size_t)(per_pass * opt.sample_count), &ro), "reserve");
    }
    std::printf("Starting to render...\n");                            // src/main.rs:1488
    const auto t0 = std::chrono::steady_clock::now();
    check(ctx, hj_render_frame(ctx, opt.sample_count, opt.seed, 0, opt.sample_count, 0, 1, &ro, &st), "render");
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const uint64_t ray_count = (uint64_t)opt.width * opt.height * opt.sample_count;   // u32 upstream (overflows), u64 here
    std::printf("Integrated %llu rays in %.6fs (%.1f rays/s)\n", (unsigned long long)ray_count, secs, (double)ray_count / secs);

    std::vector<float> rgb((size_t)opt.width * opt.height * 3);
    check(ctx, hj_framebuffer_resolve(ctx, rgb.data()), "read-back");  // Renderer::save_image, src/main.rs:1493
    save(opt.width, opt.height, rgb.data());
    if (!opt.aovs.empty()) {
      // the frame's own primary rays again (same spp and seed): sums per pixel, resolved as the Python wrapper's resolve_aovs does -
      // albedo over the sample count, normal and depth over the hit count, 0 where the count is 0
      const size_t px = (size_t)opt.width * opt.height;
      std::vector<float> aov(px * HJ_AOV_WORDS), albedo(px * 3), normal(px * 3), depth(px * 3);
      check(ctx, hj_render_aovs_frame_followed(ctx, opt.width, opt.height, opt.sample_count, opt.seed, 0, opt.sample_count, opt.aov_follow, 0u, aov.data()),
            "AOVs");
      for (size_t i = 0; i < px; i++) {
        const float* a = &aov[i * HJ_AOV_WORDS];
        const float samples = a[3], hits = a[11];
        for (int c = 0; c < 3; c++) {
          albedo[3 * i + c] = samples > 0.0f ? a[c] / samples : 0.0f;
          normal[3 * i + c] = hits > 0.0f ? a[4 + c] / hits : 0.0f;
          depth[3 * i + c] = hits > 0.0f ? a[7] / hits : 0.0f;
        }
      }
      hijiki::write_pfm(opt.aovs + "_albedo.pfm", opt.width, opt.height, albedo.data());
      hijiki::write_pfm(opt.aovs + "_normal.pfm", opt.width, opt.height, normal.data());
      hijiki::write_pfm(opt.aovs + "_depth.pfm", opt.width, opt.height, depth.data());
    }
    if (!opt.denoise.empty()) {
      // the frame's own primary rays again (same spp and seed) for the guides, then the filter over the framebuffer where it lies
      const size_t px = (size_t)opt.width * opt.height;
      std::vector<float> aov(px * HJ_AOV_WORDS), rgba(px * 4), clean(px * 3);
      check(ctx, hj_render_aovs_frame(ctx, opt.width, opt.height, opt.sample_count, opt.seed, 0, opt.sample_count, 0u, aov.data()), "AOVs");
      check(ctx, hj_denoise_frame(ctx, opt.width, opt.height, nullptr, aov.data(), &opt.denoise_opts, rgba.data()), "denoise");
      for (size_t i = 0; i < px; i++)
        for (int c = 0; c < 3; c++) clean[3 * i + c] = rgba[4 * i + c];
      save_to(opt.denoise, opt.width, opt.height, clean.data());
    }
    hj_context_destroy(ctx);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "hijiki-hip: %s\n", e.what());
    return 1;
  }
}
