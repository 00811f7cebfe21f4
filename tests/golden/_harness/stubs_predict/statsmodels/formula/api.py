OLS = Logit = None
