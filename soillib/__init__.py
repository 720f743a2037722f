"""`import soillib as soil` — the reference's Python module name
(python/soillib/__init__.py:1-3: `import silt; from .soillib import *; from .util import *`).

Live API: soillib_amd.soil (mirror of python/source/model.cpp).  Legacy API used
by example/erosion_gpu.py (map_t, data_t, erode, multiply, legacy param names,
normal): soillib_amd.legacy.  IO (tiff, geotiff): soillib_amd.io.  Helpers (`soil.util`):
soillib_amd.util.
"""
import silt  # noqa: F401

from soillib_amd.soil import *  # noqa: F401,F403
from soillib_amd.soil import (accumulate, accumulate_decay, albedo_discharge, albedo_layer,  # noqa: F401
                              albedo_stratum, d4, d8, direction, edge, gaussian_blur, gradient,
                              laplacian, layer_merge, mass_creep, mass_transfer, ms, negslope,
                              noise, noise_t, normal, ns, random_weighted, s, slope,
                              solve_uniform, steepest, timer, transport_debris, transport_fluvial,
                              us)
from soillib_amd.soil import particle_steps  # noqa: F401
from soillib_amd.soil import (accumulate_batch, direction_batch, random_weighted_batch, slope_batch,  # noqa: F401
                              steepest_batch)
from soillib_amd.soil import (basins, basins_batch, flow_length, flow_length_batch, flow_paths,  # noqa: F401
                              flow_paths_batch, watershed)
from soillib_amd.soil import (chi, downstream, downstream_batch, downstream_info, erosivity, stream_power,  # noqa: F401
                              stream_power_batch)
from soillib_amd.soil import (deposition, stream_power_deposit, stream_power_deposit_batch,  # noqa: F401
                              stream_power_deposit_info)
from soillib_amd.soil import stream_power_n, stream_power_n_batch, stream_power_n_info  # noqa: F401
from soillib_amd.soil import (stream_power_deposit_n, stream_power_deposit_n_batch,  # noqa: F401
                              stream_power_deposit_n_info)
from soillib_amd.soil import diffuse, diffuse_batch, diffuse_info  # noqa: F401
from soillib_amd.soil import (flat_distance, flat_distance_batch, flat_distance_info, flat_receivers,  # noqa: F401
                              flat_receivers_batch, resolve_flats, resolve_flats_batch)
from soillib_amd.soil import slope_limit, slope_limit_batch, slope_limit_info  # noqa: F401
from soillib_amd.soil import (mfd_accumulate, mfd_accumulate_batch, mfd_info, mfd_weights,  # noqa: F401
                              mfd_weights_batch)
from soillib_amd.soil import condition, condition_batch, fill_depressions_batch, fill_info  # noqa: F401
from soillib_amd.soil import (breach, breach_batch, condition_breached, condition_breached_batch,  # noqa: F401
                              upstream_info, upstream_length, upstream_length_batch, upstream_max,
                              upstream_max_batch, upstream_min, upstream_min_batch)
from soillib_amd.soil import (stream_magnitude, stream_magnitude_batch, stream_order,  # noqa: F401
                              stream_order_batch, stream_order_info, stream_segments, stream_segments_batch)
from soillib_amd.io import geotiff, geotiff_meta, mesh, tiff  # noqa: F401  (python/source/io.cpp:20-110)
from soillib_amd.legacy import (buffer, clamp, data_t, erode, index, map_t, multiply, param_t,  # noqa: F401
                                resize)
from soillib_amd.silt import cpu, float32, float64, gpu, int32, set, shape, tensor  # noqa: F401,A004  (legacy: soil.float32, soil.gpu, soil.set, ...)
from soillib_amd import util  # noqa: F401
