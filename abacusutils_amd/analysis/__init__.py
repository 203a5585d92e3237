from .spheres import count_in_spheres, knn_cdf, random_centres, vpf  # noqa: F401
