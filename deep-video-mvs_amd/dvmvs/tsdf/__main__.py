import sys

from dvmvs.tsdf.program import main

sys.argv[0] = "tsdf.py"       # the name the usage text has always shown for ``python -m dvmvs.tsdf`` (argparse takes it from here)
main()
