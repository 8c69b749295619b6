// Back-end boundary B1: the reference's ceres::CostFunction subclasses re-built on the HIP C ABI.
//
//   ReprojectionFactor     reference factors/reprojection_factor.h:36-158   (SizedCostFunction<2,7,7,7,1,1>)
//   ReprojectionBatch      NEW: a ceres::EvaluationCallback that evaluates ALL registered reprojection factors with one
//                          batched kernel per evaluation point; each factor's Evaluate() copies its slice out
//   ResidualBlockInfo      reference factors/residual_block_info.h:29-120
//   MarginalizationInfo    reference factors/marginalization_info.h:30-316
//   MarginalizationFactor  reference factors/marginalization_factor.h:31-105
//   Preintegration*        reference preintegration/preintegration{,_base,_normal,_earth}.{h,cc}, preintegration_factor.h
//
// There is no CPU fallback for the reprojection math: a ReprojectionFactor whose batch has not been prepared for the
// current evaluation point makes Evaluate() return false (Ceres' "evaluation failed").
//
// This header is the umbrella of the boundary: one header per subsystem, each next to the source that implements it.
#pragma once

#include "pose_sizes.h"      // POSE_LOCAL_SIZE, POSE_GLOBAL_SIZE
#include "reproj_factors.h" // HuberLossHip, ReprojectionFactor, DeviceFactorSet, ReprojectionBatch           (reproj_factors.cc)
#include "sym_eigen.h"       // symmetricEigen                                                                 (sym_eigen.cc)
#include "marg_m3.h"         // M3 on plain arrays: schurReduce, schurReduceGuarded, linearizePrior / Reduced  (marg_m3.cc)
#include "marginalization.h" // ResidualBlockInfo, MarginalizationInfo, MarginalizationFactor, the prior view  (marginalization{,_structured}.cc)
#include "preintegration.h"  // IMU, IntegrationState, Preintegration, PreintegrationFactor, PreintegrationSet (preintegration_hip.cc)
