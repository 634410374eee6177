"""reni_amd -- MI355X-native RENI forward/training hot path (HIP kernels behind the reference's
nn.Module surface).  See DESIGN.md."""
__version__ = "0.1.0"

from . import lighting  # noqa: E402,F401  (importance-sampled light lists: reni_amd.lighting.build_light_table, sample_lights, ...)
from . import glossy  # noqa: E402,F401  (prefiltered glossy lighting: reni_amd.glossy.prefilter, lookup, shade_prefiltered, ...)
