"""Measured error of the plain double library functions against the 60-digit reference at the points of tests/ad_reference.py:
maximum |value - exact| in ulp of the exact value.  A measurement of the math libraries, not of the code under test
(tanh and sech2 are this project's own compositions of expm1 and exp, csrc/hilo_ad.h::tanh_of, sech2_of).  Each side asserts
twice its own figure with a floor of 1 ulp: tests/test_ad_ops_host.py VALUE_ULPS_HOST, tests/test_ad_ops_gpu.py VALUE_ULPS
(DESIGN.md 6.1)."""
HOST_ULP = {'sin': 0.502, 'cos': 0.502, 'exp': 0.502, 'log': 0.500, 'sqrt': 0.500, 'log10': 1.359, 'asin': 0.500, 'acos': 0.500,
            'atan': 0.501, 'asinh': 0.974, 'acosh': 1.404, 'atanh': 1.364, 'tanh': 2.387, 'sech2': 2.226, 'atan2': 0.500}
DEVICE_ULP = {'sin': 0.672, 'cos': 0.630, 'exp': 0.802, 'log': 0.584, 'sqrt': 0.500, 'log10': 0.598, 'asin': 0.605, 'acos': 0.686,
              'atan': 1.155, 'asinh': 0.588, 'acosh': 0.612, 'atanh': 0.604, 'tanh': 2.387, 'sech2': 2.486, 'atan2': 1.199}
VALUE_ULPS_HOST = {f: max(1.0, 2.0 * HOST_ULP.get(f, 0.5)) for f in ('sin', 'cos', 'exp', 'log', 'sqrt', 'log10', 'asin', 'acos', 'atan',
                                                                      'asinh', 'acosh', 'atanh', 'tanh', 'sech2', 'atan2')}
VALUE_ULPS = {f: max(1.0, 2.0 * DEVICE_ULP.get(f, 0.5)) for f in ('sin', 'cos', 'exp', 'log', 'sqrt', 'log10', 'asin', 'acos', 'atan',
                                                                   'asinh', 'acosh', 'atanh', 'tanh', 'sech2', 'atan2')}
