"""Inert stand-in so pyseer.model imports where statsmodels is not installed (the predictor imports it through pyseer/model.py:14-26 and
never calls it).  Kept apart from stubs/: there it would shadow the real package for the generators that fit models."""
