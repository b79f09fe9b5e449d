from smirk_amd.expression_loss import ExpressionLoss  # noqa: F401
