"""Gumbel and survival-Gumbel copula adapters (no reference counterpart; shaped like
plackett_estimation.py).

Gumbel is upper-tail dependent; its 180-degree rotation (survival Gumbel) is lower-tail
dependent, the structure a long portfolio's loss tail needs.  One parameter theta >= 1,
2 or 3 assets (exchangeable); the device plan runs them on the SORTED strategy and takes
theta <= 16."""
from __future__ import annotations

from .... import copulas
from ._base import CopulaAdapter


class GumbelCopulaVaR(CopulaAdapter):
    copula_kind = "gumbel"
    survival = False

    @staticmethod
    def unpack_copula_params(copula_params):
        """(theta, None), as the Plackett adapter."""
        return copula_params, None

    @classmethod
    def copula_or_correl_params_insample(cls, marginals, densities):
        """The IFM fit (closed-form density)."""
        from ....optim.copula_fit import GumbelCopulaOptimizer
        return GumbelCopulaOptimizer(marginals, densities, survival=cls.survival).optimize()

    @staticmethod
    def copula_integrations_params(best_p_params):
        return best_p_params["theta"]

    @classmethod
    def copula_density(cls, cdf, nu, **kwargs):
        return copulas.gumbel(cdf, nu, survival=cls.survival)


class GumbelSurvivalCopulaVaR(GumbelCopulaVaR):
    copula_kind = "gumbel_survival"
    survival = True
