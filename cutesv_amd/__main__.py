"""python -m cutesv_amd BAM REF OUT.vcf WORK_DIR [flags]: cuteSV's command line (cutesv_amd/cli.py)"""
from .cli import main

if __name__ == "__main__":
    raise SystemExit(main())
