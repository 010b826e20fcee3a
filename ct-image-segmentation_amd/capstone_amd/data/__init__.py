"""Device-fed 2-D data: drop-in names of reference capstone/data (datasets.py, data_module.py)."""
