from .bfgs_solver import BFGSSolver
from .line_search import line_search_wolfe_conditions
from .sgd_solver import SGDSolver

__all__ = ["BFGSSolver", "SGDSolver", "line_search_wolfe_conditions"]
