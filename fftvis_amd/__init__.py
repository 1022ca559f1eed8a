"""fftvis_amd -- MI355X-native GPU backend for the fftvis visibility simulator.

Mirrors the reference package's public surface for the gpu backend
(src/fftvis/__init__.py:1-31): ``simulate_vis``, the engine / evaluator factories and the
``gpu`` sub-package; beyond it, the adjoint of ``simulate_vis`` with respect to the fluxes
(``simulate_vis_adjoint``) and a torch autograd entry point (``torch_simulate_vis``), and for basis beams the gradients
with respect to the fluxes, the coefficients and the antenna positions (``simulate_vis_basis_adjoint``,
``torch_simulate_vis_basis``, ``torch_simulate_vis_basis_array``), and the
gradient with respect to the antenna positions (``simulate_vis_position_adjoint``, ``torch_simulate_vis_array``) and to
the source positions (``simulate_vis_source_adjoint``, ``torch_simulate_vis_sky``), and the forward-mode tangent along
all three (``simulate_vis_jvp``), and the source positions through basis beams
(``simulate_vis_basis_source_adjoint``, ``simulate_vis_basis_source_jvp``, ``torch_simulate_vis_basis_sky``), and the fluxes'
and the source positions' gradients from one pass (``simulate_vis_sky_adjoint``, ``simulate_vis_basis_sky_adjoint``), and
the fit objective with its gradients from one call that keeps the visibilities on the device (``simulate_vis_chi2``,
``torch_simulate_vis_chi2``; ``simulate_vis_gain_chi2`` for uncalibrated data: per-antenna complex gains in the data model
and their gradient; ``simulate_vis_jones_chi2`` for full 2 x 2 Jones matrices per antenna, leakage included), and the
Gauss-Newton product 2 J^T W J p of that objective from one call that keeps the tangent
on the device (``simulate_vis_gauss_newton``; ``simulate_vis_gain_gauss_newton`` with the gains in the data model, a gain
direction and the gain block of the product; ``simulate_vis_jones_gauss_newton`` the same with 2 x 2 Jones matrices and a
direction of such matrices), and the gains themselves for a fixed model, solved on the device against
a resident model (``simulate_vis_gain_solve``; ``simulate_vis_jones_solve`` for the full 2 x 2 matrices), and redundant
calibration, which needs no sky: the gains together with one visibility per redundant group (``redundant_groups``,
``redundant_gain_solve``, ``redundant_average``, ``fix_redundant_degeneracies``), started on data with cable delays by
firstcal, one delay and one phase per antenna from the same redundancy (``redundant_firstcal``), and ended by absolute
calibration, which fits the amplitude and the phase gradient the data leave free to a model of the group visibilities
(``redundant_abscal``).
"""

__version__ = "0.1.0"

from .core.beams import AiryBeam, TabulatedBeam  # noqa: F401
from .core.beam_basis import compute_beam_basis, compute_beam_basis_per_freq  # noqa: F401
from .core.simulate import SimulationEngine, default_accuracy_dict  # noqa: F401
from .wrapper import create_beam_evaluator, create_simulation_engine, simulate_vis  # noqa: F401
from .adjoint import (  # noqa: F401
    antenna_to_baseline_tangent,
    baseline_to_antenna_gradient,
    radec_jacobian,
    simulate_vis_adjoint,
    simulate_vis_basis_adjoint,
    simulate_vis_basis_jvp,
    simulate_vis_basis_sky_adjoint,
    simulate_vis_basis_source_adjoint,
    simulate_vis_basis_source_jvp,
    simulate_vis_chi2,
    simulate_vis_gain_chi2,
    simulate_vis_gain_gauss_newton,
    simulate_vis_gain_solve,
    simulate_vis_gauss_newton,
    simulate_vis_jones_chi2,
    simulate_vis_jones_gauss_newton,
    simulate_vis_jones_solve,
    simulate_vis_jvp,
    simulate_vis_position_adjoint,
    simulate_vis_sky_adjoint,
    simulate_vis_source_adjoint,
    torch_simulate_vis,
    torch_simulate_vis_array,
    torch_simulate_vis_basis,
    torch_simulate_vis_basis_array,
    torch_simulate_vis_basis_sky,
    torch_simulate_vis_chi2,
    torch_simulate_vis_sky,
    topo_to_radec_gradient,
)
from .redundant import (  # noqa: F401
    fix_redundant_degeneracies,
    redundant_abscal,
    redundant_average,
    redundant_firstcal,
    redundant_gain_solve,
    redundant_groups,
)
