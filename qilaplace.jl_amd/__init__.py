"""qilaplace.jl_amd -- MI355X-native MPO x MPS apply / coefficient / compress / encode path
of QILaplace.jl, behind the reference's operator names.

The directory name contains a dot, so import it through the root-level shim:

    import qilaplace_jl_amd as qil
    psi = qil.signal_mps(x)                 # encode on the GPU
    out = W * psi                           # fused single-pass site contraction (HIP)
    qil.coefficient(out, "0101...")

Everything numeric runs in lib/libqilhip.so (HIP, gfx950); importing this package fails
loudly if that library has not been built.
"""
from ._lib import QilError, QilDomainError, LIB_PATH, last_error  # noqa: F401
from .containers import (Context, default_context, set_default_context, device_count, host_cpu_budget,  # noqa: F401
                         SignalMPS, ZTMPS, SingleSiteMPO, PairedSiteMPO)
from .ops import (apply, apply_compress, apply_compress_batch, mpo_compress, compress_batch, mpo_compress_batch, mps_block, coefficient, coefficient_batch, apply_coefficient_batch, apply_coefficient_sweep,  # noqa: F401
                  marginal_batch, coefficient_grid, laplace_values, product_batch, laplace_weights, laplace_sum, power_sum, dft_eval, dt_eval,
                  zt_eval, refine_frequencies,
                  mps_to_vector, norm, inner, environment, environment_route, shift_pencil, esprit_from_pencil, esprit, solve, solve_local_fits, solve_residual, least_squares, smooth, eigs, eigs_local_fits, eig_residual, operator_norm, condition_number, evolve, propagate, diffuse, evolve_local_fits, apply_norm, distance, apply_distance, bond_spectra, mpo_bond_spectra, entanglement_entropy,
                  truncation_error_bounds, required_maxdim, sample, apply_sample, top_k, apply_top_k, hadamard, hadamard_compress, diagonal_mpo, adjoint, convolve, correlate,
                  power_spectrum, linear_combination, linear_combination_compress, add, sub, scale, exponential_tensors,
                  mpo_linear_combination, mpo_linear_combination_compress, mpo_add, mpo_sub, mpo_scale, mpo_inner, mpo_norm,
                  mpo_distance, mpo_trace, mpo_entry_batch, mpo_slice, mpo_entries, mpo_entry, mpo_to_matrix, mpo_column, mpo_row,
                  mpo_diagonal_state, mpo_column_sums, mpo_row_sums,
                  exponential_mps, exponential_sum, restrict, zt_row, zt_column, copy_marginal, weight_batch, weight, bit_probabilities,
                  range_weight, weight_quantiles, zt_row_weights, zt_column_weights, apply_weight_batch, apply_weight,
                  apply_bit_probabilities, apply_range_weight, apply_weight_quantiles, apply_zt_row_weights, apply_zt_column_weights, canonicalize, compress, signal_mps, signal_ztmps, signal_mps_batch,
                  signal_ztmps_batch, signal_mps_cross, ztmps_from_mps, coefficient_at, coefficient_at_route, map_states, cross_map, magnitude, log_power, shrink, divide, deconvolve, rsvd,
                  svd_trunc, gemm, gemm_plan, readout_route, gemm_batched, gemm_device_time, qr_positive, qr_plan, qr_host)
from .builders import (build_qft_mpo, build_dt_mpo, build_zt_mpo, qft_mpo_tensors,  # noqa: F401
                       dt_mpo_tensors, zt_mpo_tensors, dt_mpo_tensors_many, build_dt_mpo_batch,
                       build_zt_mpo_batch, zt_qft_chain_tensors, qft_mpo_device, zt_qft_chain_device,
                       shift_mpo_tensors, build_shift_mpo, fir_mpo, laplacian_mpo_tensors, build_laplacian_mpo)
from .interchange import save, load  # noqa: F401
from .sweep import shard_items, sweep, damping_sweep, gather_results, damping_sample_bits, Comm, unshuffle  # noqa: F401

__all__ = [
    "Context", "default_context", "set_default_context", "device_count", "host_cpu_budget",
    "SignalMPS", "ZTMPS", "SingleSiteMPO", "PairedSiteMPO",
    "apply", "apply_compress", "apply_compress_batch", "coefficient", "coefficient_batch", "apply_coefficient_batch", "apply_coefficient_sweep", "marginal_batch", "coefficient_grid", "laplace_values", "mps_to_vector", "norm",
    "product_batch", "laplace_weights", "laplace_sum", "power_sum", "dft_eval", "dt_eval", "zt_eval", "refine_frequencies",
    "inner", "environment", "shift_pencil", "esprit_from_pencil", "esprit", "solve", "solve_local_fits", "solve_residual", "least_squares", "smooth", "eigs", "eigs_local_fits", "eig_residual", "operator_norm", "condition_number", "evolve", "propagate", "diffuse", "evolve_local_fits", "apply_norm", "distance", "apply_distance", "bond_spectra", "mpo_bond_spectra", "entanglement_entropy",
    "truncation_error_bounds", "required_maxdim", "sample", "apply_sample", "top_k", "apply_top_k",
    "hadamard", "hadamard_compress", "diagonal_mpo", "adjoint", "convolve", "correlate", "power_spectrum",
    "linear_combination", "linear_combination_compress", "add", "sub", "scale", "exponential_tensors", "exponential_mps",
    "mpo_linear_combination", "mpo_linear_combination_compress", "mpo_add", "mpo_sub", "mpo_scale", "mpo_inner", "mpo_norm",
    "mpo_distance", "mpo_trace", "mpo_entry_batch", "mpo_slice", "mpo_entries", "mpo_entry", "mpo_to_matrix", "mpo_column",
    "mpo_row", "mpo_diagonal_state", "mpo_column_sums", "mpo_row_sums", "shift_mpo_tensors", "build_shift_mpo", "fir_mpo", "laplacian_mpo_tensors", "build_laplacian_mpo",
    "exponential_sum", "restrict", "zt_row", "zt_column", "copy_marginal",
    "weight_batch", "weight", "bit_probabilities", "range_weight", "weight_quantiles", "zt_row_weights", "zt_column_weights",
    "apply_weight_batch", "apply_weight", "apply_bit_probabilities", "apply_range_weight", "apply_weight_quantiles", "apply_zt_row_weights",
    "apply_zt_column_weights",
    "canonicalize", "compress", "signal_mps", "signal_ztmps", "signal_mps_batch", "signal_ztmps_batch", "signal_mps_cross", "ztmps_from_mps",
    "coefficient_at", "coefficient_at_route", "map_states", "cross_map", "magnitude", "log_power", "shrink", "divide", "deconvolve",
    "rsvd", "svd_trunc", "gemm",
    "build_qft_mpo", "build_dt_mpo", "build_zt_mpo", "qft_mpo_tensors", "dt_mpo_tensors", "zt_mpo_tensors",
    "dt_mpo_tensors_many", "build_dt_mpo_batch", "build_zt_mpo_batch", "zt_qft_chain_tensors", "qft_mpo_device", "zt_qft_chain_device", "mpo_compress", "compress_batch", "mpo_compress_batch", "mps_block",
    "save", "load",
    "shard_items", "sweep", "damping_sweep", "gather_results", "damping_sample_bits", "Comm", "unshuffle",
    "QilError", "QilDomainError",
]
