"""Run the reference's predictor: python run_enet_predict.py <enet_predict args>."""
import shim  # noqa: F401  (must precede statsmodels)
from pyseer.enet_predict import main
main()
