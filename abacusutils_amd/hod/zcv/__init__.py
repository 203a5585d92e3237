"""MI355X drop-in for the heavy half of `abacusnbody.hod.zcv` (control variates).  Zel'dovich (ZCV): the Lagrangian operator
fields (`ic_fields`), their advection and the 15 field spectra (`advect_fields`) and the tracer x field spectra of one HOD
evaluation (`tracer_power.tracer_power`).  Linear (LCV, for reconstructed catalogues): the linear density spectrum and that times
mu^2 with their three spectra (`linear_fields`), the tracer-minus-randoms spectra of one HOD evaluation
(`tracer_power.recon_power`) and the field-level combination `combine_field_spectra_k3D_lcv`.  BAO reconstruction, the producer of
those catalogues, which the reference leaves to an external code (`reconstruction`: `displacement_field`, `shift`, `reconstruct`,
RecSym and RecIso in a periodic box).  The mode-coupling window file that
`run_zcv` loads (`zenbu_window.periodic_window_function`, `save_window`).  The combination with the models (`tools_cv.run_zcv`,
`run_lcv`, `run_lcv_field`; ZeNBu and classy) stays with the reference: it takes the dictionaries, grids and the window file
produced here."""
from . import advect_fields, ic_fields, linear_fields, reconstruction, tracer_power, zenbu_window  # noqa: F401
from .advect_fields import AdvectedFields, advect, field_power, lattice_positions  # noqa: F401
from .linear_fields import LinearFields, combine_field_spectra_k3D_lcv, linear_power, linear_power3d  # noqa: F401
from .reconstruction import Displacement, displacement_field, displacement_from_delta, reconstruct, shift  # noqa: F401
from .tracer_power import recon_power  # noqa: F401
from .zenbu_window import periodic_window_function, save_window  # noqa: F401

__all__ = ['ic_fields', 'advect_fields', 'tracer_power', 'linear_fields', 'zenbu_window', 'AdvectedFields', 'advect', 'field_power', 'lattice_positions',
           'LinearFields', 'linear_power', 'linear_power3d', 'combine_field_spectra_k3D_lcv', 'recon_power', 'periodic_window_function',
           'save_window', 'reconstruction', 'Displacement', 'displacement_field', 'displacement_from_delta', 'shift', 'reconstruct']
