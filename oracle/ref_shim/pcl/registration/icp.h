/* oracle/ref_shim -- empty stand-in for <pcl/registration/icp.h>: the reference's initRegistrationKSS.hpp
 * includes it and uses nothing from it (see kdtree/kdtree_flann.h).  Nothing that runs
 * pcl::IterativeClosestPoint is built against these headers: a stand-in there would be our own ICP. */
#pragma once
