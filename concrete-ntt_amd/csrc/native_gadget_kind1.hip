// fused decomposing external-product kernel instantiations: native kind 1
#define INST_KIND 1
#include "native_gadget_inst.inc"
