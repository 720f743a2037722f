// erosion_batch.hip — the twelve batch entry points of the C ABI (soil_hip.h): a step, its particle launches or
// its cell phase, each for a uniform batch, a coloured one, a parameter sweep and a batch of different models.
// Every entry describes itself in a BatchCall (common.hpp) and goes through batch_call: one set of checks in one
// order, then the phases (erosion_particles.hip: particles_batch; erosion_cells.hip: erode_cells_fused_batch).
#include <cstring>

#include "common.hpp"

using namespace soil;

namespace {

// What tells the entries apart: whose param and scale a model steps with, and which phases run.
enum BatchKind { UNIFORM, COLOURED, SWEEP, MODELS };  // MODELS: c.models is the caller's; SWEEP: c.param is B params
enum BatchPhase { PARTICLES, CELLS, STEP };

// The checks of the soil_*_batch_models entries (soil_hip.h): a NULL `models`, an N_b < 0 or >= 2^31, and what
// check_batch refuses with N = max N_b (seeds are in the records); *N_max receives max N_b.
int check_batch_models(int64_t B, int64_t H, int64_t W, const soil_batch_model* models, const char* what,
                       int64_t* N_max) {
  const std::string w(what);
  SOIL_REQUIRE(models, w + ": null models");
  int64_t N = 0;
  for (int64_t b = 0; b < B; ++b) {
    SOIL_REQUIRE(models[b].N >= 0 && models[b].N <= 0x7fffffffll,
                 w + ": models[" + std::to_string(b) + "].N outside [0, 2^31)");
    N = models[b].N > N ? models[b].N : N;
  }
  if (int rc = check_batch(B, H, W, N, &models->seed, what); rc != SOIL_OK) return rc;  // (the seeds: records)
  *N_max = N;
  return SOIL_OK;
}

// Every entry's checks, in the one order they report in: null arguments, colour planes, sizes, planes, distinct
// layer buffers.  A batch of different models leaves with c.N = max N_b (the cell phase reads no N, but refuses
// what the step refuses).
int check_batch_call(BatchCall& c, BatchKind kind, BatchPhase phase) {
  const auto msg = [&c](const char* tail) { return std::string(c.what) + tail; };
  SOIL_REQUIRE(c.P && (kind == MODELS || (c.scale && c.param)), msg(": null argument"));
  SOIL_REQUIRE(c.C ? has_colour(c.C) : kind != COLOURED, msg(": every colour plane is required"));
  if (int rc = kind == MODELS ? check_batch_models(c.B, c.H, c.W, c.models, c.what, &c.N)
                              : check_batch(c.B, c.H, c.W, c.N, c.seeds, c.what);
      rc != SOIL_OK)
    return rc;
  SOIL_REQUIRE(has_planes(*c.P, phase == PARTICLES ? PARTICLE_PLANES : STEP_PLANES),
               msg(phase == PARTICLES ? ": null plane"
                   : phase == CELLS   ? ": null plane (only `height` is optional)"
                                      : ": every plane but `height` is required"));
  SOIL_REQUIRE(phase == PARTICLES || c.P->layers != c.P->layers_next,
               msg(": layers and layers_next must be distinct buffers"));
  return SOIL_OK;
}

// The B records of a sweep: params[b] with the shared scale, N and step_index, and seeds[b] (a cells entry has no
// seeds: seed 0).
std::vector<soil_batch_model> sweep_records(const BatchCall& c) {
  std::vector<soil_batch_model> models(static_cast<size_t>(c.B));
  for (int64_t b = 0; b < c.B; ++b) {
    soil_batch_model& m = models[b];
    m.param = c.param[b];
    std::memcpy(m.scale, c.scale, sizeof(m.scale));
    m.N = c.N;
    m.seed = c.seeds ? c.seeds[b] : 0;
    m.step_index = c.step_index;
  }
  return models;
}

// An entry: the checks, then its phases, all on c.st (no internal streams: a batch fills the device by itself).  A
// step runs the two launches of the batch one after the other, then the batch's cell phase.  Records (different
// models; a sweep is a batch of different models whose records share scale, N and step_index) reach the device
// once: a step uploads them in place of the seeds of the particle phase's copy, and the cell phase reads that
// copy; a cells entry uploads them itself, in one copy.
int batch_call(BatchCall c, BatchKind kind, BatchPhase phase) {
  SOIL_DEVICE();
  if (int rc = check_batch_call(c, kind, phase); rc != SOIL_OK) return rc;
  std::vector<soil_batch_model> sweep;
  if (kind == SWEEP) {
    sweep = sweep_records(c);
    c.models = sweep.data();
  }
  const soil_batch_model* records_dev = nullptr;
  if (phase != CELLS) {
    if (int rc = particles_batch(c, phase == STEP ? &records_dev : nullptr); rc != SOIL_OK || phase == PARTICLES)
      return rc;
  } else if (c.models) {
    if (int rc = batch_models_to_device(c.models, c.B, c.st, &records_dev); rc != SOIL_OK) return rc;
  }
  return erode_cells_fused_batch(c, records_dev);
}

}  // namespace

extern "C" {

int soil_erode_step_batch(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W, int64_t N,
                          const uint64_t* seeds, uint64_t step_index, const float scale[3], const soil_param* param,
                          void* stream) {
  return batch_call({.what = "erode_step_batch", .P = planes, .B = B, .H = H, .W = W, .N = N, .seeds = seeds,
                     .step_index = step_index, .scale = scale, .param = param, .st = as_stream(stream)},
                    UNIFORM, STEP);
}

int soil_particles_batch(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W, int64_t N,
                         const uint64_t* seeds, uint64_t step_index, const float scale[3], const soil_param* param,
                         void* stream) {
  return batch_call({.what = "particles_batch", .P = planes, .B = B, .H = H, .W = W, .N = N, .seeds = seeds,
                     .step_index = step_index, .scale = scale, .param = param, .st = as_stream(stream)},
                    UNIFORM, PARTICLES);
}

int soil_erode_cells_fused_batch(const soil_erosion_planes* planes, int64_t B, int64_t H, int64_t W,
                                 const float scale[3], const soil_param* param, int flags, void* stream) {
  return batch_call({.what = "erode_cells_fused_batch", .P = planes, .B = B, .H = H, .W = W, .scale = scale,
                     .param = param, .flags = flags, .st = as_stream(stream)},
                    UNIFORM, CELLS);
}

// The coloured batch: the colour flux planes of every model cleared before the fluvial launch and the four colour
// planes carried through the cell phase.
int soil_erode_step_batch_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                 int64_t H, int64_t W, int64_t N, const uint64_t* seeds, uint64_t step_index,
                                 const float scale[3], const soil_param* param, void* stream) {
  return batch_call({.what = "erode_step_batch_colour", .P = planes, .C = colour, .B = B, .H = H, .W = W, .N = N,
                     .seeds = seeds, .step_index = step_index, .scale = scale, .param = param,
                     .st = as_stream(stream)},
                    COLOURED, STEP);
}

int soil_particles_batch_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                int64_t H, int64_t W, int64_t N, const uint64_t* seeds, uint64_t step_index,
                                const float scale[3], const soil_param* param, void* stream) {
  return batch_call({.what = "particles_batch_colour", .P = planes, .C = colour, .B = B, .H = H, .W = W, .N = N,
                     .seeds = seeds, .step_index = step_index, .scale = scale, .param = param,
                     .st = as_stream(stream)},
                    COLOURED, PARTICLES);
}

int soil_erode_cells_fused_batch_colour(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                                        int64_t B, int64_t H, int64_t W, const float scale[3],
                                        const soil_param* param, int flags, void* stream) {
  return batch_call({.what = "erode_cells_fused_batch_colour", .P = planes, .C = colour, .B = B, .H = H, .W = W,
                     .scale = scale, .param = param, .flags = flags, .st = as_stream(stream)},
                    COLOURED, CELLS);
}

// A sweep: as the (coloured) batch, model b with params[b].
int soil_erode_step_batch_params(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                 int64_t H, int64_t W, int64_t N, const uint64_t* seeds, uint64_t step_index,
                                 const float scale[3], const soil_param* params, void* stream) {
  return batch_call({.what = "erode_step_batch_params", .P = planes, .C = colour, .B = B, .H = H, .W = W, .N = N,
                     .seeds = seeds, .step_index = step_index, .scale = scale, .param = params,
                     .st = as_stream(stream)},
                    SWEEP, STEP);
}

int soil_particles_batch_params(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                int64_t H, int64_t W, int64_t N, const uint64_t* seeds, uint64_t step_index,
                                const float scale[3], const soil_param* params, void* stream) {
  return batch_call({.what = "particles_batch_params", .P = planes, .C = colour, .B = B, .H = H, .W = W, .N = N,
                     .seeds = seeds, .step_index = step_index, .scale = scale, .param = params,
                     .st = as_stream(stream)},
                    SWEEP, PARTICLES);
}

int soil_erode_cells_fused_batch_params(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                                        int64_t B, int64_t H, int64_t W, const float scale[3],
                                        const soil_param* params, int flags, void* stream) {
  return batch_call({.what = "erode_cells_fused_batch_params", .P = planes, .C = colour, .B = B, .H = H, .W = W,
                     .scale = scale, .param = params, .flags = flags, .st = as_stream(stream)},
                    SWEEP, CELLS);
}

// A batch of different models: model b with models[b].
int soil_erode_step_batch_models(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                 int64_t H, int64_t W, const soil_batch_model* models, void* stream) {
  return batch_call({.what = "erode_step_batch_models", .P = planes, .C = colour, .B = B, .H = H, .W = W,
                     .models = models, .st = as_stream(stream)},
                    MODELS, STEP);
}

int soil_particles_batch_models(const soil_erosion_planes* planes, const soil_colour_planes* colour, int64_t B,
                                int64_t H, int64_t W, const soil_batch_model* models, void* stream) {
  return batch_call({.what = "particles_batch_models", .P = planes, .C = colour, .B = B, .H = H, .W = W,
                     .models = models, .st = as_stream(stream)},
                    MODELS, PARTICLES);
}

int soil_erode_cells_fused_batch_models(const soil_erosion_planes* planes, const soil_colour_planes* colour,
                                        int64_t B, int64_t H, int64_t W, const soil_batch_model* models,
                                        int flags, void* stream) {
  return batch_call({.what = "erode_cells_fused_batch_models", .P = planes, .C = colour, .B = B, .H = H, .W = W,
                     .models = models, .flags = flags, .st = as_stream(stream)},
                    MODELS, CELLS);
}

}  // extern "C"
