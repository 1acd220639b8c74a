// see hip_runtime.h
#pragma once
