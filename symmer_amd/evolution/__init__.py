from .circuit_symmerlator import CircuitSymmerlator
from .variational_optimization import VQE_Driver, ADAPT_VQE, serialize_opt_data
