"""MI355X drop-in for the heavy half of `abacusnbody.hod.zcv` (Zel'dovich control variates): the Lagrangian operator fields
(`ic_fields`), their advection and the 15 field spectra (`advect_fields`) and the tracer x field spectra of one HOD evaluation
(`tracer_power`).  The combination with the Zel'dovich model (`tools_cv.run_zcv`, needs ZeNBu and classy) stays with the reference:
it takes the dictionaries `field_power` and `tracer_power` return."""
from . import advect_fields, ic_fields, tracer_power  # noqa: F401
from .advect_fields import AdvectedFields, advect, field_power, lattice_positions  # noqa: F401

__all__ = ['ic_fields', 'advect_fields', 'tracer_power', 'AdvectedFields', 'advect', 'field_power', 'lattice_positions']
