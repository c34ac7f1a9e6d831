import os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'xmm-superres-denoise_amd'))
from xmm_superres_denoise.engine import _lib
L=_lib.load()
for lds in (0, 65536, 80384, 81024, 81920):
    print('lds',lds,'API blocks/CU',L.xsd_debug_occupancy(lds), 'sleep-test ms: grid256 %.2f grid512 %.2f grid768 %.2f grid1024 %.2f'%tuple(L.xsd_debug_residency_ms(g,256,lds,1000) for g in (256,512,768,1024)))
