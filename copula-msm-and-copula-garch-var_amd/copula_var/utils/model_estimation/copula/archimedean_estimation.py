"""Frank, Joe and survival-Joe copula adapters (no reference counterpart; shaped like
gumbel_estimation.py).

Frank is radially symmetric without tail dependence (2 or 3 assets, where Plackett stops at 2);
Joe is upper-tail dependent with a sharper tail than Gumbel at the same Kendall tau, and its
180-degree rotation (survival Joe) lower-tail dependent.  One parameter theta -- Frank
0 < theta <= 32, Joe 1 <= theta <= 16 -- 2 or 3 assets (exchangeable); the device plan runs them
on the SORTED strategy."""
from __future__ import annotations

from .... import copulas
from ._base import CopulaAdapter


class FrankCopulaVaR(CopulaAdapter):
    copula_kind = "frank"

    @staticmethod
    def unpack_copula_params(copula_params):
        """(theta, None), as the Plackett adapter."""
        return copula_params, None

    @classmethod
    def copula_or_correl_params_insample(cls, marginals, densities):
        """The IFM fit (closed-form density)."""
        from ....optim.copula_fit import FrankCopulaOptimizer
        return FrankCopulaOptimizer(marginals, densities).optimize()

    @staticmethod
    def copula_integrations_params(best_p_params):
        return best_p_params["theta"]

    @classmethod
    def copula_density(cls, cdf, nu, **kwargs):
        return copulas.frank(cdf, nu)


class JoeCopulaVaR(CopulaAdapter):
    copula_kind = "joe"
    survival = False

    @staticmethod
    def unpack_copula_params(copula_params):
        return copula_params, None

    @classmethod
    def copula_or_correl_params_insample(cls, marginals, densities):
        from ....optim.copula_fit import JoeCopulaOptimizer
        return JoeCopulaOptimizer(marginals, densities, survival=cls.survival).optimize()

    @staticmethod
    def copula_integrations_params(best_p_params):
        return best_p_params["theta"]

    @classmethod
    def copula_density(cls, cdf, nu, **kwargs):
        return copulas.joe(cdf, nu, survival=cls.survival)


class JoeSurvivalCopulaVaR(JoeCopulaVaR):
    copula_kind = "joe_survival"
    survival = True
