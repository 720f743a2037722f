// Runs every free wrapper of include/soil.hpp (namespace silt and namespace soil; soil::erode is test_cpp_api.cpp's)
// on planes read from a directory and writes every result back, raw: tests/test_gpu_cpp_ops.py makes the inputs and
// compares each output with the CPU reference of the operation.  A wrapper that swaps two extents, hands scale.y for
// scale.x, drops an optional plane or counts its scales wrongly computes something else on these inputs — two grids
// with H != W, a batch with B, H and W pairwise different, scales (0.3, 0.7), a pair per model — and never leaves a
// buffer: every plane handed to a call has the extents the call reads.
//
//   test_cpp_ops --list    one line `OP <name>` per wrapper exercised (an overload: once per overload); no device
//   test_cpp_ops <dir>     inputs.txt + *.bin in, outputs.txt + *.bin out (tests/cpp/planes.hpp)
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <soil.hpp>

#include "planes.hpp"
#include "watchdog.hpp"

using soil::F;
using I = silt::tensor_t<int>;
using R = silt::tensor_t<silt::rng>;

#define EXPECT(c) do { if (!(c)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)
#define EXPECT_THROW(call, type) do { bool threw = false; try { call; } catch (const type&) { threw = true; } \
  if (!threw) { std::printf("FAIL %s:%d no %s from %s\n", __FILE__, __LINE__, #type, #call); return 1; } } while (0)

namespace {

// the wrappers run below; a name with overloads stands once per overload
const char* const kOps[] = {
    "check", "set", "set", "add", "multiply", "seed",
    "transport_fluvial", "transport_debris", "mass_transfer", "mass_creep", "layer_merge",
    "direction", "steepest", "random_weighted", "accumulate", "accumulate_decay", "fill_depressions", "slope",
    "flat_distance", "flat_receivers", "resolve_flats", "resolve_flats",
    "direction_batch", "steepest_batch", "random_weighted_batch", "slope_batch", "accumulate_batch",
    "flow_paths", "basins", "flow_length", "flow_paths_batch", "basins_batch", "flow_length_batch",
    "downstream", "downstream_batch", "stream_power", "stream_power_batch", "fill_depressions_batch",
    "gradient", "negslope", "laplacian", "gaussian_blur", "solve_uniform", "noise",
};

std::string g_dir;
std::map<std::string, planes::plane> g_in;
std::map<std::string, int> g_ran;

// announces the wrapper about to run (a hang names it) and counts it against kOps
void op(const char* name) {
  mark(name);
  ++g_ran[name];
}

silt::shape shape_of(const std::vector<int64_t>& d) {
  return d.size() == 1 ? silt::shape(d[0]) : d.size() == 2 ? silt::shape(d[0], d[1]) : silt::shape(d[0], d[1], d[2]);
}

template <typename T>
silt::tensor_t<T> upload(const std::string& name, const char* type) {
  const auto at = g_in.find(name);
  if (at == g_in.end()) throw std::runtime_error("no input plane " + name);
  const planes::plane& p = at->second;
  if (p.type != type) throw std::runtime_error("input plane " + name + " is " + p.type + ", wanted " + type);
  std::vector<T> v(static_cast<size_t>(p.elem()));
  std::memcpy(v.data(), p.bytes.data(), p.bytes.size());
  return silt::tensor_t<T>::from_host(v, shape_of(p.dims));
}
F f(const std::string& name) { return upload<float>(name, "f32"); }
I i(const std::string& name) { return upload<int>(name, "i32"); }

template <typename T>
std::vector<int64_t> dims_of(const silt::tensor_t<T>& t) {
  std::vector<int64_t> d;
  for (int k = 0; k < t.shape().dim(); ++k) d.push_back(t.shape()[k]);
  return d;
}
void put(const std::string& name, const F& t) { planes::write(g_dir, "outputs.txt", name, "f32", dims_of(t), t.to_host().data()); }
void put(const std::string& name, const I& t) { planes::write(g_dir, "outputs.txt", name, "i32", dims_of(t), t.to_host().data()); }
void put(const std::string& name, const R& t) {  // (seed, offset) pairs
  static_assert(sizeof(silt::rng) == 16, "soil_rng: two 64-bit words");
  planes::write(g_dir, "outputs.txt", name, "u64", {t.elem(), 2}, t.to_host().data());
}
void put(const std::string& name, const soil::flow_paths_t& p) {
  put(name + "_terminal", p.terminal);
  put(name + "_steps", p.steps);
  put(name + "_length", p.length);
}

F zeros(const silt::shape& s) {
  F t(s);
  silt::set(t, 0.0f);
  return t;
}

int run() {
  const silt::vec2 sc{0.3f, 0.7f};
  const silt::vec3 sc3{0.3f, 0.7f, 4.0f};
  const std::vector<silt::vec2> per{{0.3f, 0.7f}, {1.1f, 0.4f}, {0.25f, 3.0f}}, one{{0.6f, 0.2f}};
  const double dt = 3.5;
  const struct { soil::edge_t e; const char* s; } edges[] = {{soil::D4, "d4"}, {soil::D8, "d8"}};

  // ---- silt ----------------------------------------------------------------------------------------------
  {
    F sf(silt::shape(7, 9));
    I si(silt::shape(7, 9));
    op("set"); silt::set(sf, 3.5f);
    op("set"); silt::set(si, -4);
    put("set_f", sf);
    put("set_i", si);
    F a = f("sa"), b = f("sb"), m = f("sa");
    op("add"); silt::add(a, b);
    op("multiply"); silt::multiply(m, 0.5f);
    put("add", a);
    put("multiply", m);
    R r(silt::shape(100));
    op("seed"); silt::seed(r, 42, 1000);
    put("seed", r);
  }

  // ---- what needs no reference -----------------------------------------------------------------------------
  mark("in-binary checks");
  {
    EXPECT_THROW(silt::tensor_t<float>(silt::shape(4, 4), silt::CPU), silt::error::mismatch_host);
    const F h = f("h_a"), hb = f("hb");
    const std::vector<uint64_t> two{3, 5};  // one seed short of the batch
    op("check");  // the C ABI's refusal comes back as the reference's exception
    EXPECT_THROW(soil::steepest(h, soil::edge_t(7)), std::invalid_argument);
    EXPECT_THROW(soil::steepest_batch(hb, soil::edge_t(7)), std::invalid_argument);
    EXPECT_THROW(soil::random_weighted_batch(hb, soil::D8, two, 7, 10.0f), std::invalid_argument);
    const std::vector<float> vf{1.5f, -0.0f, 3e38f, 1e-44f, 7.0f, -2.25f};
    EXPECT(std::memcmp(F::from_host(vf, silt::shape(2, 3)).to_host().data(), vf.data(), sizeof(float) * vf.size()) == 0);
    const std::vector<int> vi{-1, 0, 2147483647, -2147483647 - 1, 5};
    EXPECT(I::from_host(vi, silt::shape(5)).to_host() == vi);
    const std::vector<silt::rng> vr{{1, 2}, {~0ull, 0}, {3, ~0ull}};
    const std::vector<silt::rng> back = R::from_host(vr, silt::shape(3)).to_host();
    EXPECT(back.size() == vr.size());
    for (size_t k = 0; k < vr.size(); ++k) EXPECT(back[k].seed == vr[k].seed && back[k].offset == vr[k].offset);
  }

  // ---- the two grids: a = 12 x 20 (rows of whole four-cell windows), b = 13 x 21 ------------------------------
  for (const char* g : {"a", "b"}) {
    const std::string G = std::string("_") + g;
    const F h = f("h" + G), src = f("src" + G), decay = f("decay" + G);
    const I stop = i("stop" + G);
    const F ca = f("ca" + G), cb = f("cb" + G), ct = f("ct" + G), k = f("k" + G), up = f("up" + G);
    for (const auto& ed : edges) {
      const soil::edge_t e = ed.e;
      const std::string T = G + "_" + ed.s;
      const I graph = i("graph" + T);
      op("direction"); put("direction" + T, soil::direction(h, e));
      op("steepest"); put("steepest" + T, soil::steepest(h, e));
      op("random_weighted"); put("random_weighted" + T, soil::random_weighted(h, e, 3, 7, 10.0f));
      op("accumulate"); put("accumulate" + T, soil::accumulate(graph, src, e));
      op("accumulate_decay"); put("accumulate_decay" + T, soil::accumulate_decay(graph, src, decay, e));
      op("fill_depressions"); put("fill_depressions" + T, soil::fill_depressions(h, e));
      op("flat_distance"); put("flat_distance" + T, soil::flat_distance(h, e));
      op("flat_receivers"); put("flat_receivers" + T, soil::flat_receivers(graph, h, i("dist" + T), e));
      op("resolve_flats"); put("resolve_flats_graph" + T, soil::resolve_flats(h, e, i("rwgraph" + T)));
      op("resolve_flats"); put("resolve_flats" + T, soil::resolve_flats(h, e));
      op("flow_paths"); put("flow_paths_stop" + T, soil::flow_paths(graph, e, sc, stop));
      op("flow_paths"); put("flow_paths" + T, soil::flow_paths(graph, e, sc));
      op("basins"); put("basins_stop" + T, soil::basins(graph, e, stop));
      op("basins"); put("basins" + T, soil::basins(graph, e));
      op("flow_length"); put("flow_length_stop" + T, soil::flow_length(graph, e, sc, stop));
      op("flow_length"); put("flow_length" + T, soil::flow_length(graph, e, sc));
      op("downstream"); put("downstream_all" + T, soil::downstream(graph, e, ca, cb, ct, &sc, stop));
      op("downstream"); put("downstream" + T, soil::downstream(graph, e));
      op("stream_power"); put("stream_power_all" + T, soil::stream_power(h, graph, k, e, sc, dt, up, stop));
      op("stream_power"); put("stream_power" + T, soil::stream_power(h, graph, k, e, sc, dt));
    }
    op("slope"); put("slope" + G, soil::slope(h, i("graph" + G + "_d8"), sc));
    op("gradient"); put("gradient" + G, soil::gradient(h, sc));
    op("negslope"); put("negslope" + G, soil::negslope(h, sc));
    for (const char* c : {"1", "2"}) {  // channels
      op("laplacian"); put("laplacian" + std::string(c) + G, soil::laplacian(f("t" + std::string(c) + G), sc));
      F t = f("t" + std::string(c) + G);
      op("gaussian_blur");
      F ret = soil::gaussian_blur(t, 3.0f);
      EXPECT(ret.data() == t.data());  // blurs in place and returns its input's handle
      put("gaussian_blur" + std::string(c) + G, t);
      R r(silt::shape(700));
      op("seed"); silt::seed(r, 5, 100);
      op("solve_uniform");
      put("solve_uniform" + std::string(c) + G, soil::solve_uniform(f("flow" + G), f("source" + std::string(c) + G), f("sudecay" + G), r, sc, 700));
    }
    // the cell ops: mass_transfer with the colour planes, mass_creep on a delta of its own, layer_merge
    const F layers = f("layers" + G);
    F delta = f("delta" + G), surface = f("albedo_surface" + G);
    const silt::shape hw(layers.shape()[0], layers.shape()[1]);
    op("mass_transfer");
    soil::mass_transfer(delta, layers, f("uplift" + G), zeros(hw), f("mass" + G), f("momentum" + G), f("debris" + G),
                        zeros(layers.shape()), f("albedo_bedrock" + G), f("albedo_fluvial" + G), f("albedo_debris" + G),
                        surface, sc3, soil::param_t());
    put("mass_transfer_delta" + G, delta);
    put("mass_transfer_surface" + G, surface);
    F creep = f("delta" + G);
    op("mass_creep"); soil::mass_creep(creep, layers, sc3, soil::param_t());
    put("mass_creep" + G, creep);
    F merged(hw);
    op("layer_merge"); soil::layer_merge(merged, layers);
    put("layer_merge" + G, merged);
    soil::noise_param_t np;
    np.seed = 3.0f; np.ext[0] = float(hw[0]); np.ext[1] = float(hw[1]);
    op("noise"); put("noise" + G, soil::noise(hw, np));
  }

  // ---- the batch: B = 3 models of 12 x 20 ------------------------------------------------------------------------
  {
    const F hb = f("hb"), srcb = f("srcb"), decayb = f("decayb");
    const I stopb = i("stopb");
    const F ca = f("cab"), cb = f("cbb"), ct = f("ctb"), k = f("kb"), up = f("upb");
    const std::vector<uint64_t> seeds{3, 5, 9};
    for (const auto& ed : edges) {
      const soil::edge_t e = ed.e;
      const std::string T = std::string("_") + ed.s;
      const I graph = i("graphb" + T);
      op("direction_batch"); put("direction_batch" + T, soil::direction_batch(hb, e));
      op("steepest_batch"); put("steepest_batch" + T, soil::steepest_batch(hb, e));
      op("random_weighted_batch"); put("random_weighted_batch" + T, soil::random_weighted_batch(hb, e, seeds, 7, 10.0f));
      op("accumulate_batch"); put("accumulate_batch_decay" + T, soil::accumulate_batch(graph, srcb, e, decayb));
      op("accumulate_batch"); put("accumulate_batch" + T, soil::accumulate_batch(graph, srcb, e));
      op("fill_depressions_batch"); put("fill_depressions_batch" + T, soil::fill_depressions_batch(hb, e));
      op("flow_paths_batch"); put("flow_paths_batch_stop" + T, soil::flow_paths_batch(graph, e, per, stopb));
      op("flow_paths_batch"); put("flow_paths_batch" + T, soil::flow_paths_batch(graph, e, one));
      op("basins_batch"); put("basins_batch_stop" + T, soil::basins_batch(graph, e, stopb));
      op("basins_batch"); put("basins_batch" + T, soil::basins_batch(graph, e));
      op("flow_length_batch"); put("flow_length_batch_stop" + T, soil::flow_length_batch(graph, e, per, stopb));
      op("flow_length_batch"); put("flow_length_batch" + T, soil::flow_length_batch(graph, e, one));
      op("downstream_batch"); put("downstream_batch_all" + T, soil::downstream_batch(graph, e, ca, cb, ct, per, stopb));
      op("downstream_batch"); put("downstream_batch_one" + T, soil::downstream_batch(graph, e, ca, cb, ct, one));
      op("downstream_batch"); put("downstream_batch" + T, soil::downstream_batch(graph, e));
      op("stream_power_batch"); put("stream_power_batch_all" + T, soil::stream_power_batch(hb, graph, k, e, per, dt, up, stopb));
      op("stream_power_batch"); put("stream_power_batch" + T, soil::stream_power_batch(hb, graph, k, e, one, dt));
    }
    const I graph = i("graphb_d8");
    op("slope_batch"); put("slope_batch_per", soil::slope_batch(hb, graph, per));
    op("slope_batch"); put("slope_batch_one", soil::slope_batch(hb, graph, one));
  }

  // ---- the particle launches: 33 x 50, 700 walkers, default parameters, generators seeded here -----------------
  {
    const F layers = f("tp_layers");
    const silt::shape hw(layers.shape()[0], layers.shape()[1]), hw2(hw[0], hw[1], 2), hw3(hw[0], hw[1], 3);
    const silt::vec3 s3{20.0f / float(hw[0]), 20.0f / float(hw[1]), 4.0f};
    {
      F wh = f("tf_discharge"), wf = zeros(hw), m = zeros(hw), mf = zeros(hw), v = f("tf_momentum"), vf = zeros(hw2), af = zeros(hw3);
      R r(silt::shape(700));
      op("seed"); silt::seed(r, 5, 100);
      op("transport_fluvial");
      soil::transport_fluvial(layers, f("tf_rainfall"), wh, wf, m, mf, v, vf, F(), af, f("tf_albedo"), r, s3, soil::param_t());
      put("tf_discharge", wh); put("tf_discharge_track", wf); put("tf_mass", m); put("tf_mass_track", mf);
      put("tf_momentum", v); put("tf_momentum_track", vf); put("tf_albedo_track", af); put("tf_rng", r);
    }
    {
      F v = f("td_velocity"), vf = zeros(hw2), m = zeros(hw), mf = zeros(hw), af = zeros(hw3);
      R r(silt::shape(700));
      op("seed"); silt::seed(r, 6, 9);
      op("transport_debris");
      soil::transport_debris(layers, v, vf, m, mf, F(), af, f("td_albedo"), r, s3, soil::param_t());
      put("td_velocity", v); put("td_velocity_track", vf); put("td_mass", m); put("td_mass_track", mf);
      put("td_albedo_track", af); put("td_rng", r);
    }
  }

  // every wrapper of the list has run, an overloaded name at least once per overload
  mark("the list against what ran");
  std::map<std::string, int> listed;
  for (const char* name : kOps) ++listed[name];
  for (const auto& l : listed) EXPECT(g_ran[l.first] >= l.second);
  for (const auto& r : g_ran) EXPECT(listed.count(r.first) == 1);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "--list") == 0) {
    for (const char* name : kOps) std::printf("OP %s\n", name);
    return 0;
  }
  if (argc != 2) {
    std::printf("usage: test_cpp_ops --list | <dir>\n");
    return 2;
  }
  start_watchdog(60.0);  // a hang becomes exit code 3 with the last marker, not a killed child without output
  g_dir = argv[1];
  try {
    mark("reading the inputs");  // on the host alone: a plane of the wrong size is refused on any machine
    g_in = planes::read_all(g_dir, "inputs.txt");
    std::remove((g_dir + "/outputs.txt").c_str());
    mark("device count");
    if (soil_device_count() == 0) {  // no CPU fallback: the first allocation must throw
      try { silt::tensor_t<float> t(silt::shape(4, 4)); } catch (const std::runtime_error&) {
        std::printf("NO_DEVICE_OK\n"); return 0; }
      return 1;
    }
    if (const int rc = run()) return rc;
  } catch (const std::exception& e) {
    std::printf("FAIL exception in \"%s\": %s\n", g_marker.load(), e.what());
    return 1;
  }
  std::printf("CPP_OPS_WALL %.3f\n", since_start());
  std::printf("CPP_OPS_OK\n");
  mark(kExitMarker);
  return 0;
}
