/* oracle/ref_shim -- stand-in for <pcl/point_cloud.h> (TEST INFRASTRUCTURE, see kdtree/kdtree_flann.h).
 * A container with the four members the reference's two headers use; it has no behaviour. */
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

namespace pcl {

template <typename PointT>
class PointCloud {
public:
    typedef std::shared_ptr<PointCloud<PointT> > Ptr;
    typedef std::shared_ptr<const PointCloud<PointT> > ConstPtr;

    std::vector<PointT> points;
    std::uint32_t width;
    std::uint32_t height;

    PointCloud() : width(0), height(0) {}
};

}  // namespace pcl
