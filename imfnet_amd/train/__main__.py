import sys

from .trainer import main

sys.exit(main())
