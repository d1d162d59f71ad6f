from .circuit_symmerlator import CircuitSymmerlator
from .variational_optimization import VQE_Driver, ADAPT_VQE, serialize_opt_data
from .time_evolution import evolve_state, chebyshev_coefficients, spectral_interval, EvolutionResult
from .exponentiation import exponentiate_single_Pop, trotter, truncated_exponential
