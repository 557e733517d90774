"""voronoirt_amd -- MI355X-native formal solver behind VoronoiRT's driver surface.

Only what the hot path needs: the C-ABI library (csrc/ -> libvrt_hip.so), the host-side mirror
of the reference interface (api.py), seeded synthetic grids (synth.py) and the one-process-per-GPU
sharding of the angle x wavelength loop (distributed.py).  Importing this package does not
load the shared library; the first call does, and fails loudly if it is missing.
"""
from .api import (Delaunay_downII, Delaunay_upII, FormalPlan, J_lambda_voronoi, VoronoiSites,  # noqa: F401
                  direction, quadrature_directions, read_cell, read_quadrature, voro, voro_dev, QUADRATURE_DIR,
                  short_characteristics_batch, short_characteristics_down, short_characteristics_up,
                  RegularSolver, LineCase, Lambda_voronoi, Lambda_voronoi_host, J_lambda_voronoi_line, MultiDevicePlan,
                  Lambda_regular, J_lambda_regular_line,
                  nearest_sites, Voronoi_to_Raster, Voronoi_to_Raster_inv_dist, initialise, Voronoi_to_Raster_dev,
                  initialise_dev, raster_stats, rejection_sampling, rejection_sampling_dev, sample_from_invNH_invT,
                  sample_from_logNH_invT, sample_from_logNH_invT_rootv, sample_from_temp_gradient, periodic_axis,
                  synth_opacity, synth_opacity_dev, top_intensity, top_intensity_dev, tau_unity, tau_unity_dev,
                  emergent_spectrum, ContinuumCase, Lambda_continuum, Lambda_continuum_regular, continuum_update_dev,
                  lambda_diagonal, continuum_ali_update_dev, lambda_diagonal_regular, line_lambda_diagonal,
                  line_lambda_diagonal_regular, lambda_ali_update_dev, lambda_ali_update_native_dev)
from ._lib import VrtError  # noqa: F401

__all__ = ["Delaunay_upII", "Delaunay_downII", "FormalPlan", "J_lambda_voronoi", "VoronoiSites",
           "direction", "quadrature_directions", "read_cell", "read_quadrature", "voro", "voro_dev", "VrtError",
           "QUADRATURE_DIR", "short_characteristics_up", "short_characteristics_down",
           "short_characteristics_batch", "RegularSolver", "LineCase", "Lambda_voronoi", "Lambda_voronoi_host",
           "J_lambda_voronoi_line", "MultiDevicePlan", "Lambda_regular", "J_lambda_regular_line", "nearest_sites", "Voronoi_to_Raster",
           "Voronoi_to_Raster_inv_dist", "initialise", "Voronoi_to_Raster_dev", "initialise_dev", "raster_stats",
           "rejection_sampling", "rejection_sampling_dev", "sample_from_invNH_invT", "sample_from_logNH_invT",
           "sample_from_logNH_invT_rootv", "sample_from_temp_gradient", "periodic_axis", "synth_opacity",
           "synth_opacity_dev", "top_intensity", "top_intensity_dev", "tau_unity", "tau_unity_dev", "emergent_spectrum",
           "ContinuumCase", "Lambda_continuum", "Lambda_continuum_regular", "continuum_update_dev", "lambda_diagonal",
           "continuum_ali_update_dev", "lambda_diagonal_regular", "line_lambda_diagonal", "line_lambda_diagonal_regular",
           "lambda_ali_update_dev", "lambda_ali_update_native_dev"]
