from .bispectrum import bispectrum_from_spectrum, calc_bispectrum, triangle_counts  # noqa: F401
from .groups import fof_groups, group_properties, group_sizes, linking_lengths, multiplicity_function  # noqa: F401
from .lensing import ProjectedParticles, delta_sigma, delta_sigma_box, delta_sigma_from_sums, projected_sums  # noqa: F401
from .minkowski import (calc_minkowski, gaussian_prediction, mesh_moments, minkowski_counts, minkowski_from_counts,  # noqa: F401
                        minkowski_functionals)
from .mst import minimum_spanning_tree, mst_branches, mst_statistics  # noqa: F401
from .spheres import count_in_spheres, knn_cdf, random_centres, vpf  # noqa: F401
from .threepcf import calc_3pcf, triplet_multipoles, zeta_from_counts  # noqa: F401
from .voids import find_voids, find_voids_mesh, tophat_smooth, void_galaxy_xi, void_size_function  # noqa: F401
from .watershed import (find_watershed_voids, merge_zones, persistence_pairs, watershed_mesh, watershed_size_function, zone_galaxy_xi,  # noqa: F401
                        zone_hierarchy)
