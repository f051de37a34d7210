// Empty stand-in: nms_kernel.cu includes this THC header but uses nothing from it (oracle/thc_shim/THC/THC.h).
#pragma once
