#!/bin/bash
# build_variant.sh NAME FILE.hip [extra hipcc flags...] — development aid: links a variant of the library in which one source is compiled
# with extra flags (e.g. -DGRT_FWD_WAVES=3) into variants/libgrut_amd_NAME.so; select it with GRUT_AMD_LIB=...  (3dgrut_amd/build.py: variant)
exec python "$(dirname "$0")/../3dgrut_amd/build.py" --variant "$@"
