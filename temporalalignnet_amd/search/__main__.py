"""`python -m temporalalignnet_amd.search ...`"""
from .cli import main

raise SystemExit(main())
