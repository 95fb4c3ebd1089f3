"""python -m fresco_amd.ebsynth: the reference Ebsynth binary's command line on the HIP backend."""
import sys

from . import main

sys.exit(main())
